"""The C-ABI shared library loads on a CPU-only box and exports every symbol include/va.h declares
(no compute calls: there is no GPU here and no CPU fallback in the library); the binding's signature table, struct mirrors
and restated constants are held to the header's text."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    from video_analytics_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        __graft_entry__.build()
    return _ffi.lib()


def test_every_declared_symbol_is_exported(lib):
    from video_analytics_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "va.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(va_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_ffi.EXPORTS), declared ^ set(_ffi.EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.va_version() >= 1


def _header():
    """include/va.h without its comments."""
    text = open(os.path.join(ROOT, "include", "va.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "//" not in text  # the header is C89-commented throughout; a // comment would hide text from the parsers below
    return text


def _mirrors():
    """The header's struct names and the ctypes mirrors of video_analytics_amd._ffi."""
    from video_analytics_amd import _ffi
    return {"va_tvl1_params": _ffi.Tvl1Params, "va_tvl1_options": _ffi.Tvl1Options, "va_tvl1_launch": _ffi.Tvl1Launch,
            "va_brox_params": _ffi.BroxParams, "va_farneback_params": _ffi.FarnebackParams, "va_dtraj_params": _ffi.DenseTrajParams,
            "va_stip_params": _ffi.StipParams, "va_gmm_params": _ffi.GmmParams, "va_kmeans_params": _ffi.KmeansParams,
            "va_solver": _ffi.SolverParams}


_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
            "unsigned long long": ctypes.c_ulonglong}
_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "void": None, "const char*": ctypes.c_char_p}
_HANDLES = ("void", "va_ctx", "va_vgg16")


def _prototypes(hdr):
    """[(name, return type, [argument, ...])] of every function the header declares, in its order.  What is left of the header
    once the preprocessor lines, the extern "C" braces, the struct and enum definitions are taken out is cut at every ';',
    and each piece must be a prototype: one that does not parse fails here."""
    text = re.sub(r"^[ \t]*#.*$", "", hdr, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', "", text)
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{[^{}]*\}\s*\w+\s*;", "", text)
    text = re.sub(r"typedef\s+struct\s+\w+\s+\w+\s*;", "", text)
    text = re.sub(r"enum\s*\{[^{}]*\}\s*;", "", text)
    out = []
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if stmt in ("", "}"):  # "}" closes extern "C"
            continue
        m = re.fullmatch(r"([a-z_ ]+\*?) ?\b(va_[a-z0-9_]+) ?\(([^()]+)\)", stmt)
        assert m, "not a prototype: %r" % stmt
        args = m.group(3).strip()
        out.append((m.group(2), m.group(1).strip(), [] if args == "void" else [a.strip() for a in args.split(",")]))
    return out


def _allowed(arg, mirrors):
    """The ctypes types an argument declared as ``arg`` may be bound as."""
    stars = arg.count("*")
    words = re.sub(r"\bconst\b|\*", " ", arg).split()
    assert len(words) >= 2 and re.fullmatch(r"[A-Za-z_]\w*", words[-1]), "unnamed or unparsed argument %r" % arg
    base = " ".join(words[:-1])
    assert base in _SCALARS or base in _HANDLES or base in mirrors or base == "char", "unknown type in %r" % arg
    if stars >= 2:
        return (ctypes.POINTER(ctypes.c_void_p),)
    if stars == 0:
        return (_SCALARS[base],)  # a struct, void or char by value is a KeyError: the ABI has none
    if base == "char":
        return (ctypes.c_char_p,)
    if base in _HANDLES:
        return (ctypes.c_void_p,)
    if base in mirrors:
        return (ctypes.POINTER(mirrors[base]),)
    return (ctypes.c_void_p, ctypes.POINTER(_SCALARS[base]))  # a device buffer, or a host array of exactly that scalar


def test_signature_table_equals_the_header():
    """Every row of _ffi.SIGNATURES against the prototype include/va.h declares: the same functions in the same order, the
    return type, the argument count and every argument's type.  A device buffer may be bound as c_void_p whatever scalar
    the header points it at; everything else has one legal ctypes type.  Needs no library."""
    from video_analytics_amd import _ffi
    hdr = _header()
    protos = _prototypes(hdr)
    names = [p[0] for p in protos]
    scanned = re.findall(r"\b(va_[a-z0-9_]+)\s*\(", hdr)  # test_every_declared_symbol_is_exported's scan
    assert names == scanned and len(set(names)) == len(names)  # no prototype is left out, none twice
    assert list(_ffi.SIGNATURES) == names, [(a, b) for a, b in zip(_ffi.SIGNATURES, names) if a != b][:3] or (
        set(names) ^ set(_ffi.SIGNATURES))
    assert _ffi.EXPORTS == names
    mirrors = _mirrors()
    assert set(mirrors) == set(re.findall(r"typedef\s+struct\s+(\w+)\s*\{", hdr))  # every struct of the header has a mirror
    bad = []
    for name, ret, args in protos:
        restype, argtypes = _ffi.SIGNATURES[name]
        if restype is not _RETURNS[ret]:
            bad.append("%s returns %s, bound as %s" % (name, ret, restype))
        if len(argtypes) != len(args):
            bad.append("%s takes %d arguments, bound with %d" % (name, len(args), len(argtypes)))
            continue
        for i, (arg, bound) in enumerate(zip(args, argtypes)):
            if not any(bound is t for t in _allowed(arg, mirrors)):
                bad.append("%s argument %d, %r, bound as %s" % (name, i, arg, bound.__name__))
    assert not bad, "\n".join(bad)


def _c_name(field):
    return "lambda" if field == "lambda_" else field  # the one rename: lambda is a Python keyword


def test_struct_mirrors_have_the_header_layout(tmp_path):
    """sizeof, and offsetof and size of every field, of the ten structs as the C compiler lays include/va.h out, against
    the ctypes mirrors.  A field the header lacks does not compile; a field the mirror lacks changes sizeof.  The program
    calls no library function and links against nothing."""
    import shutil
    import subprocess
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    mirrors = _mirrors()
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "va.h"', 'int main(void) {']
    want = []
    for cname, cls in mirrors.items():
        lines.append('    printf("%s %%lu\\n", (unsigned long)sizeof(%s));' % (cname, cname))
        want.append("%s %d" % (cname, ctypes.sizeof(cls)))
        for field, _ in cls._fields_:
            c = _c_name(field)
            lines.append('    printf("%s.%s %%lu %%lu\\n", (unsigned long)offsetof(%s, %s), (unsigned long)sizeof(((%s*)0)->%s));'
                         % (cname, c, cname, c, cname, c))
            want.append("%s.%s %d %d" % (cname, c, getattr(cls, field).offset, getattr(cls, field).size))
    lines += ['    return 0;', '}', '']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want) == sum(1 + len(cls._fields_) for cls in mirrors.values())
    bad = ["header: %s   mirror: %s" % (g, w) for g, w in zip(got, want) if g != w]
    assert not bad, "(name, [offset,] size)\n" + "\n".join(bad)


def test_restated_constants_equal_the_header():
    """Every #define and enum constant of include/va.h that _ffi restates has the header's value."""
    from video_analytics_amd import _ffi
    hdr = _header()
    value = {k: int(v, 0) for k, v in re.findall(r"^[ \t]*#define[ \t]+(VA_\w+)[ \t]+(-?\w+)[ \t]*$", hdr, flags=re.M)}
    for body in re.findall(r"enum\s*\{([^{}]*)\}", hdr):
        for item in body.split(","):
            k, v = item.split("=")  # every enumerator of the header states its value
            assert k.strip() not in value
            value[k.strip()] = int(v, 0)
    same = ["VA_OK", "VA_ERR_INVALID", "VA_ERR_HIP", "VA_ERR_WORKSPACE", "VA_ERR_STOPPED", "VA_COLOR_JITTER_PARTIALS",
            "VA_GMM_SOFT", "VA_GMM_HARD", "VA_BOW_NONE", "VA_BOW_L1", "VA_BOW_L2"]
    same += [k for k in value if k.startswith("VA_OPT_")]
    assert sorted(k for k in value if k.startswith("VA_ERR_")) == sorted(same[1:5])
    got = {k: getattr(_ffi, k) for k in same}
    got.update({"VA_STIP_MAX_" + k: getattr(_ffi, "STIP_MAX_" + k) for k in ("SIGMAS", "TAUS", "RADIUS")})
    got.update({"VA_TVL1_LAUNCH_" + k.upper(): i for i, k in enumerate(_ffi.TVL1_LAUNCH_FAMILIES)})
    assert sorted(k for k in value if k.startswith("VA_TVL1_LAUNCH_")) == sorted(k for k in got if k.startswith("VA_TVL1_LAUNCH_"))
    bad = ["%s is %d in va.h, %r in _ffi" % (k, value[k], v) for k, v in got.items() if value[k] != v or type(v) is not int]
    assert not bad, "\n".join(bad)
    # every name of the module that looks like a header constant is one of the checked ones
    assert {k for k in vars(_ffi) if k.startswith("VA_")} == set(same)


def test_host_only_entry_points(lib):
    from oracle import tvl1_oracle
    from video_analytics_amd import _ffi
    p = _ffi.default_tvl1_params()
    assert (round(p.tau, 4), round(p.lambda_, 4), round(p.theta, 4), p.nscales, p.warps, p.iters) == (0.25, 0.15, 0.3, 5, 5, 300)
    assert abs(p.epsilon - 0.01) < 1e-9 and abs(p.scale_step - 0.8) < 1e-7 and p.block_iters == 0 and p.fast_math == 0 and p.tile_mask == 0
    from video_analytics_amd.flow import pyramid_sizes
    for (w, h) in [(224, 224), (1280, 720), (320, 240), (64, 48), (17, 300)]:
        assert pyramid_sizes(w, h) == tvl1_oracle.pyramid_sizes(w, h)
    assert pyramid_sizes(224, 224) == [(224, 224), (179, 179), (143, 143), (114, 114), (91, 91)]
    assert sum(a * b for a, b in pyramid_sizes(1280, 720)) == 2285258
    assert lib.va_tvl1_workspace_bytes(224, 224, 32, 11, ctypes.byref(p)) > 0
    assert lib.va_tvl1_workspace_bytes(8, 8, 1, 2, ctypes.byref(p)) == 0  # too small: rejected
    assert b"out of range" in lib.va_last_error()


def test_pyramid_sizes_equal_the_oracle_over_steps_and_depths(lib):
    """va_tvl1_pyramid_sizes against the oracle's (host arithmetic on both sides): sizes at and just above the 16-pixel
    minimum, odd sizes, every scale step the GPU tests use, nscales up to and above the 16 levels both sides clamp to."""
    from oracle import tvl1_oracle
    from video_analytics_amd import _ffi, flow
    sizes = (16, 17, 20, 40, 224, 333, 1280)
    deepest = 0
    for step in (0.1, 0.2, 0.5, 0.65, 0.8, 0.9, 0.95):
        for nscales in (1, 5, 16, 40):
            p = _ffi.default_tvl1_params(scale_step=step, nscales=nscales)
            for w in sizes:
                for h in sizes:
                    got = flow.pyramid_sizes(w, h, p)
                    assert got == tvl1_oracle.pyramid_sizes(w, h, nscales, step), (w, h, step, nscales)
                    assert 1 <= len(got) <= min(nscales, 16) and got[0] == (w, h) and min(min(s) for s in got) >= 16
                    deepest = max(deepest, len(got))
    assert deepest == 16  # the clamp of nscales = 40 is reached (1280 x 1280 at step 0.9 and 0.95)
    assert len(flow.pyramid_sizes(56, 40, _ffi.default_tvl1_params(scale_step=0.95, nscales=40))) == 16


BAD_TVL1_PARAMS = [
    (dict(scale_step=0.0), "scale_step"), (dict(scale_step=1.0), "scale_step"), (dict(scale_step=float("nan")), "scale_step"),
    (dict(tau=0.0), "must be > 0"), (dict(tau=-0.25), "must be > 0"), (dict(tau=float("nan")), "must be > 0"),
    (dict(lambda_=0.0), "must be > 0"), (dict(lambda_=-0.15), "must be > 0"), (dict(lambda_=float("nan")), "must be > 0"),
    (dict(theta=0.0), "must be > 0"), (dict(theta=-0.3), "must be > 0"), (dict(theta=float("nan")), "must be > 0"),
    (dict(tau=1.0, theta=0.0005), "<= 1000"),      # tau / theta = 2000
    (dict(lambda_=100.0, theta=20.0), "<= 1000"),  # lambda * theta = 2000 (tau / theta = 0.0125)
    (dict(nscales=0), "must be >= 1"),
]


@pytest.mark.parametrize("over,msg", BAD_TVL1_PARAMS, ids=[",".join("%s=%s" % kv for kv in o.items()) for o, _ in BAD_TVL1_PARAMS])
def test_workspace_bytes_rejects_bad_tvl1_parameters(lib, over, msg):
    """va_tvl1_workspace_bytes answers 0 and leaves a message naming the parameter (flow.tvl1_flow turns exactly that into
    its ValueError: tests/test_tvl1_params_gpu.py, the call needs a device); the neighbouring legal values are accepted."""
    from video_analytics_amd import _ffi
    p = _ffi.default_tvl1_params(**over)
    assert lib.va_tvl1_workspace_bytes(64, 64, 1, 2, ctypes.byref(p)) == 0, over
    assert msg in lib.va_last_error().decode(), (over, lib.va_last_error())
    for ok in (dict(scale_step=0.1), dict(scale_step=0.95), dict(tau=1.0, theta=0.001), dict(lambda_=100.0, theta=10.0), dict(nscales=1),
               dict(nscales=40)):
        assert lib.va_tvl1_workspace_bytes(64, 64, 1, 2, ctypes.byref(_ffi.default_tvl1_params(**ok))) > 0, ok


def test_ctx_create_fails_loudly_without_a_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from video_analytics_amd import _ffi, flow
    with pytest.raises(RuntimeError):
        _ffi.ctx(0)
    with pytest.raises((RuntimeError, ValueError)):
        flow.tvl1_flow(torch.zeros(1, 2, 64, 64, dtype=torch.uint8))


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "video_analytics_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".inc")):
                src = open(os.path.join(dp, f)).read()
                assert "oracle" not in src.replace("no oracle", ""), os.path.join(dp, f)


def test_tile_plan_of_the_benchmark_pyramid():
    """Host-side tiling logic of va_tvl1_flow (no GPU needed): the plan documented in profiles/README.md for the
    224x224 benchmark pyramid in fixed-iteration mode, and the epsilon mode's forced block depth 1."""
    from video_analytics_amd import _ffi, flow
    plan = flow.tile_plan(224, 224, _ffi.default_tvl1_params(epsilon=0.0))
    # the 224^2, 179^2, 143^2 (two 128-column strips each) and 114^2 (one strip) levels stream through FOUR waves (round 3): 4 x 4
    # levels = 16 iterations per pass, 4 x 5 = 20 on 179^2 and 143^2, where a 20-column halo still costs no third strip;
    # 91^2 (too few jobs) iterates on 64x64 register tiles -- the measured choice
    assert [(d["tile_w"], d["tile_h"], d["waves"], d["block_iters"], d["tiles_x"]) for d in plan] == [
        (128, 0, 4, 16, 2), (128, 0, 4, 20, 2), (128, 0, 4, 20, 2), (128, 0, 4, 16, 1), (64, 64, 4, 16, 2)]
    # (143^2 streams too since the last strips of two pairs share a wave: 1.5 strips per pair, 74 % full; without the sharing
    # -- tile_mask bit 10 -- it stays on the register tiles)
    plain = flow.tile_plan(224, 224, _ffi.default_tvl1_params(epsilon=0.0, tile_mask=1 << 10))
    assert [(d["tile_w"], d["tile_h"], d["waves"], d["block_iters"], d["tiles_x"]) for d in plain] == [
        (128, 0, 4, 16, 2), (128, 0, 4, 20, 2), (64, 64, 4, 12, 3), (128, 0, 4, 16, 1), (64, 64, 4, 16, 2)]
    two = flow.tile_plan(224, 224, _ffi.default_tvl1_params(epsilon=0.0, stream_waves=2))  # the two-wave form of rounds 1-2
    assert [(d["tile_w"], d["tile_h"], d["waves"], d["block_iters"], d["tiles_x"]) for d in two] == [
        (128, 0, 2, 16, 2), (128, 0, 2, 16, 2), (64, 64, 4, 12, 3), (128, 0, 2, 16, 1), (64, 64, 4, 16, 2)]
    # the switches of the retired kernel families are refused loudly instead of silently running something else
    for kw in (dict(tile_mask=1 << 9), dict(stream_ppl=3), dict(stream_waves=3), dict(stream_waves=4), dict(stream_waves=5), dict(stream_waves=6), dict(stream_waves=10), dict(stream_waves=12), dict(stream_queue=1),
               dict(rows_levels=1), dict(rows_cfg=40)):
        assert _ffi.lib().va_tvl1_workspace_bytes(224, 224, 1, 2, _ffi.default_tvl1_params(epsilon=0.0, **kw)) == 0, kw
        assert b"VA_EXPERIMENTS" in _ffi.lib().va_last_error()
    everywhere = flow.tile_plan(224, 224, _ffi.default_tvl1_params(epsilon=0.0, tile_mask=1 << 8))
    assert [(d["tile_w"], d["tiles_x"]) for d in everywhere] == [(128, 2), (128, 2), (128, 2), (128, 1), (128, 1)]
    hd = flow.tile_plan(1280, 720, _ffi.default_tvl1_params(epsilon=0.0))  # wide levels: four waves x 3 levels, 12 per pass, halo 12
    assert [(d["tile_w"], d["waves"], d["block_iters"], d["tiles_x"]) for d in hd] == [
        (128, 4, 12, 13), (128, 4, 12, 10), (128, 4, 12, 8), (128, 4, 12, 7), (128, 4, 12, 5)]
    hd1 = flow.tile_plan(1280, 720, _ffi.default_tvl1_params(epsilon=0.0, stream_waves=1))  # one wave, 10 per pass, halo 10
    assert [(d["tile_w"], d["waves"], d["block_iters"], d["tiles_x"]) for d in hd1] == [
        (128, 1, 10, 12), (128, 1, 10, 10), (128, 1, 10, 8), (128, 1, 10, 6), (128, 1, 10, 5)]
    plan = flow.tile_plan(224, 224, _ffi.default_tvl1_params(epsilon=0.0, tile_mask=0xFF))  # register tiles only
    assert [(d["tile_w"], d["tile_h"], d["waves"], d["block_iters"]) for d in plan] == [
        (64, 64, 4, 12), (64, 64, 4, 12), (64, 64, 4, 12), (128, 64, 8, 7), (64, 64, 4, 16)]
    assert [(d["tiles_x"], d["tiles_y"]) for d in plan] == [(5, 5), (4, 4), (3, 3), (1, 2), (2, 2)]
    for d, n in zip(plan, (224, 179, 143, 114, 91)):  # the valid regions of the tiles cover the level
        hx = -(-d["block_iters"] // 4) * 4 if d["tiles_x"] > 1 else 0
        assert d["tiles_x"] * d["tile_w"] - 2 * hx * (d["tiles_x"] - 1) >= n
        hy = d["block_iters"] if d["tiles_y"] > 1 else 0
        assert d["tiles_y"] * d["tile_h"] - 2 * hy * (d["tiles_y"] - 1) >= n
    assert all(d["block_iters"] == 1 for d in flow.tile_plan(224, 224, _ffi.default_tvl1_params(epsilon=0.01)))
    forced = flow.tile_plan(224, 224, _ffi.default_tvl1_params(epsilon=0.0, block_iters=6, tile_mask=1 << 5))
    assert all((d["tile_w"], d["tile_h"], d["block_iters"]) == (128, 32, 6) for d in forced)


def test_tvl1_plans_equal_the_recorded_ones(lib):
    """tile_plan and va_tvl1_workspace_bytes over a grid of frame sizes, pair counts and tuning values reproduce
    tests/golden/tvl1_plans.npz exactly: the file was recorded from the library before the row pipeline's host side was
    reduced to one launch helper and one description of the pipeline shape (tests/golden/make_tvl1_plan_golden.py)."""
    import importlib.util
    import numpy as np
    path = os.path.join(ROOT, "tests", "golden", "make_tvl1_plan_golden.py")
    spec = importlib.util.spec_from_file_location("make_tvl1_plan_golden", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert os.path.getsize(gen.OUT) < 100 * 1024
    want, got = np.load(gen.OUT), gen.compute()
    assert sorted(want.files) == sorted(got)
    for name in want.files:
        assert want[name].dtype == got[name].dtype and want[name].shape == got[name].shape, name
        bad = np.argwhere(want[name] != got[name])
        assert len(bad) == 0, "%s differs at %d places, first at index %s" % (name, len(bad), bad[0])
    assert int(got["levels"].min()) >= 1 and int(got["workspace"].min()) > 0  # every case of the grid is an accepted one


def test_flow_plans_equal_the_recorded_ones(lib):
    """va_brox_workspace_bytes, va_farneback_workspace_bytes and flow.pyramid_sizes through a BroxParams and a FarnebackParams,
    over a grid of frame sizes, sequence and frame counts, scale steps, level counts and kernel shapes, reproduce
    tests/golden/flow_plans.npz exactly: the file was recorded from the library before the three methods' front end became
    one (tests/golden/make_flow_plan_golden.py)."""
    import importlib.util
    import numpy as np
    path = os.path.join(ROOT, "tests", "golden", "make_flow_plan_golden.py")
    spec = importlib.util.spec_from_file_location("make_flow_plan_golden", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert os.path.getsize(gen.OUT) < 100 * 1024
    want, got = np.load(gen.OUT), gen.compute()
    assert sorted(want.files) == sorted(got)
    for name in want.files:
        assert want[name].dtype == got[name].dtype and want[name].shape == got[name].shape, name
        bad = np.argwhere(want[name] != got[name])
        assert len(bad) == 0, "%s differs at %d places, first at index %s" % (name, len(bad), bad[0])
    for method in ("brox", "farneback"):  # every case of the grid is an accepted one, in the recording too
        for g in (want, got):
            assert int(g[method + "_levels"].min()) >= 1 and int(g[method + "_workspace"].min()) > 0, method


def test_public_header_is_plain_c(tmp_path):
    """include/va.h is a C ABI: it must compile as C99 (no C++ or torch types) with the system compiler."""
    import shutil
    import subprocess
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "va.h"\nint main(void) { va_tvl1_params p; va_tvl1_default_params(&p); return va_version() > 0 ? 0 : 1; }\n')
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_integration_md_quotes_the_executed_binding_stub():
    """INTEGRATION.md section 1 shows tests/reference_binding_stub.py verbatim (the file tests/test_binding_stub_gpu.py
    executes): the documented reference-side binding is tested code."""
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    stub = open(os.path.join(ROOT, "tests", "reference_binding_stub.py")).read()
    assert "```python\n" + stub + "```" in md
