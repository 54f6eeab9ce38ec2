"""Which TV-L1 kernel ran: every case names the launches it exists for, and is compared with the oracle.

``flow.launch_plan`` (``va_tvl1_launch_plan``) is the level, chunk, warp and iteration loop of ``va_tvl1_flow_opt`` running
dry: one record per inner-iteration and median launch.  ``_properties`` turns a report into named properties (kernel
instantiations, pair chunks, strips, chunks of rows, shared last strips, pass shapes, remainder launches, layout
conversions between levels, the median option); nothing else feeds them.  A case of ``CASES`` gives a frame size, sequences
x frames, parameters and ``must``, the properties it exists for.  Its GPU test
  * asserts ``must`` <= the properties of the report,
  * asserts that the launches ``flow.profile_levels`` counted per level during the run equal the report's,
  * compares the flow bit for bit with the C oracle (``tests/tvl1_median_oracle.c`` with the median option).
``FAST_CASES`` do the same for ``fast_math = 1`` (1-ulp arithmetic, no oracle): every form equals the register tiles' result
bit for bit, the forced candidates with the stopping rule equal each other, and in fixed-iteration mode the result stays
within 1e-3 px of the oracle, the bound of ``test_streaming_kernel_fast_math_and_mixed_levels``.

CPU tests (no GPU): ``must`` holds for every case's report; the instantiations ``launch_iter``, ``launch_stream`` and
``launch_median`` of tvl1.hip can launch (32 + 10 + 2) are exactly those the two tables name; every property of the plans of
the benchmark's and BASELINE.md's workloads (with and without ``median = 5``) is reached by a case of ``CASES``.

Findings (what the report showed when the claims of tests/test_tvl1_row_pipeline_paths_gpu.py and of
``test_every_register_tile_candidate_bit_exact`` became assertions):
  * 224 x 40 with 37 iterations was claimed to run the 4 x 4 pipeline; 37 = 3 passes of 12, below the 13 a 4 x 4 pass needs to
    end in its last wave, so it ran 2 x 8 + 2 x 8 + 1 x 10.  179 x 33 with 41 iterations ("4 x 5; passes of unequal K") ran
    2 x 8 three times for the same reason (41 = 3 x 13 < 16), 143 x 30 with 41 likewise, and 114 x 30 with 33 ran 2 x 8 + 2 x 8 +
    1 x 10.  No four-wave pass of unequal K was compared with the oracle on these frames.  The frames stay (their true
    properties are asserted there now); ``rows_*`` below keep each frame and move the iteration count to the smallest one
    that reaches the claimed path (45 = 15 + 15 + 15, 37 = 19 + 18, ...).
  * 130 x 24 ("last strip two columns wide", 4 x 5 in one pass of 16 with shared last strips) and 300 x 20 ("three strips",
    which its 25 iterations run in the one-wave form: 4 x 3 over three strips is ``rows_300x20_three_strips`` at 23) ran what
    they claim.
  * A fallback pass after four-wave passes happens only with the median option (a short last segment); no test had one:
    ``rows_224x40_median_fallback_after_four_wave``.
  * The eight forced candidates of 300 x 150 each ran alone on both levels, in both modes, with several tiles and halos in
    x and y: the claim holds (``pick_tiles``' allow-all fallback is not taken there).
  * Never compared with the oracle before: a pair-chunked launch beyond chunk 0 (``pair0 > 0`` in k_warp, k_iter_tile,
    k_median and k_median_store; only the 320-pair property test ran one), chunks with the median option, and a chunked tile
    level feeding a streaming level.  Never launched by any test: ``k_iter_tile<..., EPS = true, FAST = true>`` (all eight
    candidates) and, with ``FAST = true`` without the stopping rule, every candidate but the default pick's.
  * No wrong result: every new case was bit-exact on the first run.

Measured on the MI355X: the 59 GPU tests of this file take 5 s together, oracle included; the slowest are
chunks3_forced_256x16_median5 (1.0 s, 67 M pixel-iterations through the median oracle) and chunks2_tile_into_stream_114_median3
(0.64 s); every row-pipeline and fast-math case is below 0.05 s.  The 62 CPU tests take 2 s.
"""
import collections
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tuning fields of va_tvl1_params the oracle has no counterpart for (results must not depend on them)
PRODUCT_ONLY = ("block_iters", "tile_mask", "stream_levels", "stream_waves", "stream_chunks", "stream_slots", "stream_ppl",
                "stream_queue", "rows_levels", "rows_cfg", "fast_math", "median", "median_every")
FAST_BOUND = 1e-3  # px, max |fast - exact| in fixed-iteration mode (tests/test_tvl1_gpu.py)


def _case(W, H, S, F, must, **kw):
    return dict(W=W, H=H, S=S, F=F, kw=kw, must=tuple(must))


def _tile(c, eps=0, fast=0):
    return "k_iter_tile<c%d,EPS=%d,FAST=%d>" % (c, eps, fast)


def _stream(waves, levels, fast=0):
    return "k_iter_stream<%dx%d,FAST=%d>" % (waves, levels, fast)


ROWS = dict(epsilon=0.0, warps=2, nscales=1, tile_mask=1 << 8)  # tests/test_tvl1_row_pipeline_paths_gpu.py, 3 pairs
CAND = dict(epsilon=0.0, iters=17, warps=2, nscales=2, block_iters=5)  # test_every_register_tile_candidate_bit_exact
CAND_EPS = dict(epsilon=0.02, iters=40, warps=1, nscales=2)

# id -> case.  must: the properties of the report the case exists for (_properties).
CASES = {
    # ---- pair chunks: the smallest frames and pair counts whose report shows the property (a chunk needs more than 283 pairs of 91 x 91)
    "chunks3_forced_256x16": _case(128, 128, 145, 3, [_tile(4), "only_c4", "pair_chunks=3", "ragged_pair_chunk", "pair_chunk_splits_sequence",
                                                      "pair_chunks_with_warps>1", "short_last_tile_launch_own_grid"],
                                   epsilon=0.0, nscales=1, iters=7, warps=2, block_iters=3, tile_mask=1 << 4),
    "chunks3_forced_256x16_median5": _case(128, 128, 145, 3, [_tile(4), "k_median<5>", "pair_chunks=3", "median_with_pair_chunks",
                                                              "median_short_last_segment", "median_on_tile_level"],
                                           epsilon=0.0, nscales=1, iters=7, warps=2, block_iters=3, tile_mask=1 << 4, median=5, median_every=4),
    "chunks2_default_91": _case(91, 91, 145, 3, [_tile(7), "pair_chunks=2", "pair_chunk_splits_sequence", "pitch_padding:tile",
                                                 "short_last_tile_launch_own_halo"],
                                epsilon=0.0, nscales=1, iters=40, warps=1),  # (14 + 14 + 12 iterations, halo 16, 16, 12)
    "chunks2_tile_into_stream_114": _case(114, 114, 145, 3, [_tile(7), _stream(2, 8), "pair_chunks=2", "chunked_tile_level_into_stream_level",
                                                             "tile_level_into_stream_level", "strips=1"],
                                          epsilon=0.0, nscales=2, iters=10, warps=2),
    "chunks2_tile_into_stream_114_median3": _case(114, 114, 145, 3, ["k_median<3>", "pair_chunks=2", "median_with_pair_chunks",
                                                                     "median_on_tile_level", "median_on_stream_level", "median_short_last_segment",
                                                                     "chunked_tile_level_into_stream_level"],
                                                  epsilon=0.0, nscales=2, iters=10, warps=2, median=3, median_every=4),
    # ---- the six frames of tests/test_tvl1_row_pipeline_paths_gpu.py at iteration counts that reach the claimed path
    "rows_224x40_two_strips_4x4": _case(224, 40, 3, 2, [_stream(4, 4), "strips=2", "only_four_wave"], iters=45, **ROWS),
    "rows_224x40_uneven_4x4": _case(224, 40, 3, 2, [_stream(4, 4), "strips=2", "uneven_passes", "only_four_wave"], iters=44, **ROWS),
    "rows_179x33_4x5_uneven": _case(179, 33, 3, 2, [_stream(4, 5), "strips=2", "uneven_passes", "pitch_padding:stream"], iters=37, **ROWS),
    "rows_143x30_shared_last_strips": _case(143, 30, 3, 2, [_stream(4, 5), "narrow", "narrow_odd_pairs", "strips=2"], iters=37, **ROWS),
    "rows_130x24_last_strip_two_columns": _case(130, 24, 3, 2, [_stream(4, 5), "narrow", "narrow_odd_pairs", "two_columns_past_one_strip"], iters=16, **ROWS),
    "rows_114x30_single_strip": _case(114, 30, 3, 2, [_stream(4, 4), "strips=1", "uneven_passes"], iters=31, **ROWS),
    "rows_300x20_three_strips": _case(300, 20, 3, 2, [_stream(4, 3), "strips>=3", "uneven_passes"], iters=23, **ROWS),
    # ---- chunks of rows under shared last strips (the 320 x 240 and 1280 x 720 plans): two chunks of 36 and 35 rows
    "rows_256x71_narrow_row_chunks": _case(256, 71, 3, 2, [_stream(4, 3), "strips>=3", "narrow", "narrow_odd_pairs", "row_chunks>1",
                                                           "short_last_row_chunk", "narrow_with_row_chunks"], iters=23, stream_chunks=2, **ROWS),
    "rows_224x40_median_fallback_after_four_wave": _case(224, 40, 3, 2, [_stream(4, 4), _stream(1, 10), "fallback_pass_after_four_wave", "mixed_waves",
                                                                         "median_on_stream_level", "k_median<3>", "median_short_last_segment"],
                                                         iters=20, median=3, median_every=16, **ROWS),
    # ---- and as the old file runs them (what the report says they reach)
    "rows_224x40_37_fallback": _case(224, 40, 3, 2, [_stream(2, 8), _stream(1, 10), "one_wave_remainder", "strips=2", "no_four_wave"], iters=37, **ROWS),
    "rows_179x33_41_fallback": _case(179, 33, 3, 2, [_stream(2, 8), "strips=2", "no_four_wave"], iters=41, **ROWS),
    "rows_143x30_41_fallback": _case(143, 30, 3, 2, [_stream(2, 8), "strips=2", "no_four_wave", "pitch_padding:stream"], iters=41, **ROWS),
    "rows_114x30_33_fallback": _case(114, 30, 3, 2, [_stream(2, 8), _stream(1, 10), "one_wave_remainder", "strips=1", "no_four_wave"], iters=33, **ROWS),
    "rows_300x20_25_one_wave": _case(300, 20, 3, 2, [_stream(1, 10), "strips>=3", "no_four_wave"], iters=25, **ROWS),
    "rows_224x40_one_wave": _case(224, 40, 3, 2, [_stream(1, 10), "strips=2"], iters=37, stream_waves=1, **ROWS),
    "rows_224x40_two_waves": _case(224, 40, 3, 2, [_stream(2, 8), _stream(1, 10), "strips=2"], iters=37, stream_waves=2, **ROWS),
}
for _bit in range(8):
    CASES["cand%d_300x150" % _bit] = _case(300, 150, 1, 3, [_tile(_bit), "only_c%d" % _bit, "c%d:tiles_x>1" % _bit, "c%d:tiles_y>1" % _bit,
                                                            "c%d:halo_x" % _bit, "short_last_tile_launch"], tile_mask=1 << _bit, **CAND)
    CASES["cand%d_300x150_eps" % _bit] = _case(300, 150, 1, 3, [_tile(_bit, eps=1), "only_c%d" % _bit, "eps", "c%d:tiles_x>1" % _bit,
                                                                "c%d:tiles_y>1" % _bit, "c%d:halo_x" % _bit], tile_mask=1 << _bit, **CAND_EPS)

# fast_math = 1.  group: the cases of a group run the same frames and schedule and must agree bit for bit.
FAST_CASES = {}
for _bit in range(8):
    FAST_CASES["fast_cand%d_eps" % _bit] = dict(_case(300, 150, 1, 3, [_tile(_bit, eps=1, fast=1), "only_c%d" % _bit, "eps", "fast"],
                                                      tile_mask=1 << _bit, fast_math=1, **CAND_EPS), group="cand_eps")
    FAST_CASES["fast_cand%d" % _bit] = dict(_case(300, 150, 1, 3, [_tile(_bit, fast=1), "only_c%d" % _bit, "fast"],
                                                  tile_mask=1 << _bit, fast_math=1, **CAND), group="cand")
for _sw, (_nw, _kh) in {1: (1, 10), 2: (2, 8), 7: (4, 4), 8: (4, 5), 9: (4, 3)}.items():
    FAST_CASES["fast_stream_%dx%d" % (_nw, _kh)] = dict(_case(131, 57, 3, 2, [_stream(_nw, _kh, fast=1), "fast"], epsilon=0.0, iters=40, warps=2,
                                                              nscales=2, tile_mask=1 << 8, stream_waves=_sw, fast_math=1), group="stream")
FAST_CASES["fast_stream_tiles"] = dict(_case(131, 57, 3, 2, ["fast", "no_stream"], epsilon=0.0, iters=40, warps=2, nscales=2, tile_mask=0xFF,
                                             fast_math=1), group="stream")

# The workloads whose plans CASES must reach property by property: bench.py (224 x 224, 32 clips of 11 frames as one call and
# as two calls of 16 on two streams), BASELINE.md's 320 x 240 clips in the same two forms and its 1280 x 720 configuration (16
# pairs), each with the default parameters (fixed iterations) and again with median = 5.
WORKLOADS = [(224, 224, 32, 11), (224, 224, 16, 11), (320, 240, 32, 11), (320, 240, 16, 11), (1280, 720, 16, 2)]


# ------------------------------------------------------------------------------------------- report -> properties ----

def _inst(r):
    if r["family"] == "tile":
        return _tile(r["cfg"], r["eps"], r["fast"])
    if r["family"] == "stream":
        return _stream(r["waves"], r["levels"], r["fast"])
    return "k_median<%d>" % r["median"]


def _properties(plan, F):
    """The named properties of a report (list of dicts of flow.launch_plan) of a call with F frames per sequence."""
    props = set()
    levels = collections.OrderedDict()
    for r in plan:
        levels.setdefault(r["level"], []).append(r)
        props.add(_inst(r))
    kind = {s: next(r["family"] for r in recs if r["family"] != "median") for s, recs in levels.items()}
    cands = {r["cfg"] for r in plan if r["family"] == "tile"}
    if len(cands) == 1:
        props.add("only_c%d" % min(cands))
    props.add("no_stream" if "stream" not in kind.values() else "streams")
    for s, recs in levels.items():
        it = [r for r in recs if r["family"] != "median"]
        med = [r for r in recs if r["family"] == "median"]
        assert all(r["family"] == kind[s] for r in it), "one kernel family per level"
        chunks = sorted({(r["pair0"], r["npairs"]) for r in recs})
        # the chunks tile the pairs of the call, in order
        assert chunks[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(chunks, chunks[1:])), chunks
        if len(chunks) > 1:
            assert kind[s] == "tile", "only register-tile levels run chunk by chunk"
            props.add("pair_chunks=%d" % len(chunks))
            if len({n for _, n in chunks}) > 1:
                props.add("ragged_pair_chunk")
            if any(p0 % (F - 1) for p0, _ in chunks):
                props.add("pair_chunk_splits_sequence")
            if any(r["warp"] > 0 for r in recs):
                props.add("pair_chunks_with_warps>1")
            if med:
                props.add("median_with_pair_chunks")
            if kind.get(s - 1) == "stream":
                props.add("chunked_tile_level_into_stream_level")
        if s - 1 in kind and kind[s - 1] != kind[s]:
            props.add("%s_level_into_%s_level" % (kind[s], kind[s - 1]))
        if recs[0]["pitch"] != recs[0]["w"]:
            props.add("pitch_padding:" + kind[s])
        for r in med:
            props.add("median_on_%s_level" % kind[s])
        # segments: the launches of one warp of one chunk between two filters
        segs = collections.OrderedDict()
        seg = -1
        for r in recs:
            key = (r["pair0"], r["warp"])
            if r["family"] == "median" or key + (seg,) not in segs:
                seg += 1
            if r["family"] != "median":
                segs.setdefault(key + (seg,), []).append(r)
        lens = collections.defaultdict(list)
        for (p0, wp, _), rs in segs.items():
            lens[(p0, wp)].append(sum(r["K"] for r in rs))
            assert [r["it0"] for r in rs] == list(np.cumsum([rs[0]["it0"]] + [r["K"] for r in rs[:-1]])), "iterations in order"
        for ls in lens.values():
            if med and ls[-1] < ls[0]:
                props.add("median_short_last_segment")
        for rs in segs.values():
            if kind[s] == "stream":
                four = [r for r in rs if r["waves"] == 4]
                if len({r["K"] for r in four}) > 1:
                    props.add("uneven_passes")
                for a, b in zip(rs, rs[1:]):
                    if a["waves"] == 2 and b["waves"] == 1:
                        props.add("one_wave_remainder")
            else:
                first, last = rs[0], rs[-1]
                if last["K"] < first["K"]:
                    props.add("short_last_tile_launch")
                    if last["halo_x"] != first["halo_x"]:
                        props.add("short_last_tile_launch_own_halo")
                    if (last["cfg"], last["grid_x"]) != (first["cfg"], first["grid_x"]):
                        props.add("short_last_tile_launch_own_grid")
        for (p0, wp) in lens:
            rs = [r for r in it if (r["pair0"], r["warp"]) == (p0, wp)]
            if any(a["waves"] == 4 and b["waves"] < 4 for a, b in zip(rs, rs[1:]) if kind[s] == "stream"):
                props.add("fallback_pass_after_four_wave")
        for r in it:
            if r["family"] == "stream":
                assert r["grid_y"] == (-(-r["npairs"] // 2) if r["narrow"] else r["npairs"]), r
                assert r["grid_x"] == ((2 * r["strips"] - 1) if r["narrow"] else r["strips"]) * r["row_chunks"], r
                assert (r["row_chunks"] - 1) * r["rows_per_chunk"] < r["h"] <= r["row_chunks"] * r["rows_per_chunk"], r
                props.add("strips=%d" % r["strips"] if r["strips"] <= 2 else "strips>=3")
                if r["row_chunks"] > 1:
                    props.add("row_chunks>1")
                    if r["h"] % r["rows_per_chunk"]:
                        props.add("short_last_row_chunk")
                    if r["narrow"]:
                        props.add("narrow_with_row_chunks")
                if r["narrow"]:
                    props.add("narrow")
                    if r["npairs"] % 2:
                        props.add("narrow_odd_pairs")
                if r["strips"] == 2 and r["w"] - 128 <= 2:
                    props.add("two_columns_past_one_strip")
            else:
                assert r["grid_x"] == r["strips"] * r["row_chunks"] and r["grid_y"] == r["npairs"], r
                if r["strips"] > 1:
                    props.add("c%d:tiles_x>1" % r["cfg"])
                if r["row_chunks"] > 1:
                    props.add("c%d:tiles_y>1" % r["cfg"])
                if r["halo_x"] > 0:
                    props.add("c%d:halo_x" % r["cfg"])
        if kind[s] == "stream":
            props.add("only_four_wave" if all(r["waves"] == 4 for r in it) else "no_four_wave" if all(r["waves"] < 4 for r in it) else "mixed_waves")
    for r in plan:
        if r["eps"]:
            props.add("eps")
        if r["fast"]:
            props.add("fast")
    return props


def _plan(case):
    from video_analytics_amd import flow as vflow
    return vflow.launch_plan(case["W"], case["H"], case["S"], case["F"], **case["kw"])


def assert_claims(cid):
    """``must`` of case ``cid`` holds for its report (also called by the older TV-L1 tests for the frames they share)."""
    case = dict(CASES, **FAST_CASES)[cid]
    props = _properties(_plan(case), case["F"])
    assert set(case["must"]) <= props, (cid, sorted(set(case["must"]) - props), sorted(props))
    return props


# ------------------------------------------------------------------------------------------------ coverage (CPU) ----

@pytest.mark.parametrize("cid", sorted(CASES) + sorted(FAST_CASES))
def test_report_has_the_properties_the_case_exists_for(cid):
    """CPU: the dry run of the launch loop reports every property of ``must``."""
    assert_claims(cid)


def launchable_instantiations():
    """The instantiations tvl1.hip's launch_iter, launch_stream and launch_median can launch, in this file's names."""
    src = open(os.path.join(ROOT, "video_analytics_amd", "csrc", "tvl1.hip")).read()
    src = re.sub(r"//[^\n]*", "", src)

    def body(name):
        m = re.search(r"^[^\n;]*\b%s\([^)]*\)\s*\{(.*?)^\}" % name, src, flags=re.S | re.M)
        assert m, name
        return m.group(1)

    consts = {k: int(v) for k, v in re.findall(r"constexpr int (kStream\w+) = (\d+);", src)}
    cfgs = re.search(r"constexpr TileCfg kCfgs\[\] = \{(.*?)\};", src, flags=re.S).group(1)
    cfgs = [tuple(map(int, c)) for c in re.findall(r"\{(\d+), (\d+), (\d+), (\d+)\}", cfgs)]
    out = set()
    # launch_iter<EPS, FAST>: one k_iter_tile per candidate, whose template arguments are the candidate's waves and lanes in x
    tiles = re.findall(r"(case (\d+)|default):\s*k_iter_tile<2, 4, (\d+), (\d+), EPS, FAST><<<grid, (\d+), 0, st>>>", body("launch_iter"))
    assert len(tiles) == len(cfgs) == 8
    for i, (_, case_no, nw, lx, threads) in enumerate(tiles):
        assert case_no in ("", str(i)) and cfgs[i][2:] == (int(nw), int(lx)) and int(threads) == 64 * int(nw), (i, cfgs[i])
    flags = set(re.findall(r"launch_iter<(true|false), (true|false)>\(", src))
    assert len(flags) == 4
    for i in range(8):
        for e, f in flags:
            out.add(_tile(i, int(e == "true"), int(f == "true")))
    # launch_stream: the shapes it dispatches to, each with FAST true and false
    b = body("launch_stream")
    assert "k_iter_stream<2, KH, NWV, true>" in b and "k_iter_stream<2, KH, NWV, false>" in b and len(re.findall(r"k_iter_stream<", b)) == 2
    shapes = re.findall(r"return go\(integral_constant<int, (\w+)>\{\}, integral_constant<int, (\w+)>\{\}\)", b)
    assert len(shapes) == len(re.findall(r"return go\(", b)) == 5
    for nw, kh in shapes:
        for f in (0, 1):
            out.add(_stream(int(nw), consts[kh] if kh in consts else int(kh), f))
    b = body("launch_median")
    meds = re.findall(r"k_median<(\d)><<<", b)
    assert len(meds) == len(re.findall(r"<<<", b)) == 2
    out |= {"k_median<%s>" % k for k in meds}
    # nothing else launches these kernels
    for kernel, n in (("k_iter_tile<", 8), ("k_iter_stream<", 2), ("k_median<", 2)):
        assert len(re.findall(re.escape(kernel) + r"[^;{}]*<<<", src)) == n, kernel
    return out


def _is_instantiation(name):
    return name.startswith(("k_iter_tile<", "k_iter_stream<", "k_median<"))


def test_every_launched_instantiation_is_named_by_a_case():
    """CPU: the instantiations the case tables name in ``must`` (each asserted from the report and run on the GPU) are exactly
    the 32 + 10 + 2 that launch_iter, launch_stream and launch_median can launch."""
    launchable = launchable_instantiations()
    assert len(launchable) == 44
    named = {m for c in list(CASES.values()) + list(FAST_CASES.values()) for m in c["must"] if _is_instantiation(m)}
    assert named == launchable, sorted(named ^ launchable)


def test_every_property_of_the_workload_plans_is_reached_by_a_case():
    """CPU: whatever the reports of the benchmark's and BASELINE.md's default-parameter calls show, with and without
    median = 5, a case of CASES shows too (and is compared with the oracle).  A plan that gains a property fails here."""
    from video_analytics_amd import flow as vflow
    reached = set()
    for case in CASES.values():
        reached |= _properties(_plan(case), case["F"])
    for (W, H, S, F) in WORKLOADS:
        for opts in (dict(), dict(median=5)):
            plan = vflow.launch_plan(W, H, S, F, epsilon=0.0, **opts)
            missing = _properties(plan, F) - reached
            assert not missing, ((W, H, S, F, opts), sorted(missing))


def test_the_benchmark_call_chunks_its_coarsest_level_and_the_dry_run_counts_it():
    """CPU: the report of the 320-pair call (a single-stream benchmark step): the 91 x 91 level runs as two chunks of 160 pairs, every
    other level in one; the records are complete (5 levels x 5 warps x 300 iterations each) and a counting call agrees."""
    import ctypes
    from video_analytics_amd import _ffi, flow as vflow
    plan = vflow.launch_plan(224, 224, 32, 11, epsilon=0.0)
    chunks = {s: sorted({(r["pair0"], r["npairs"]) for r in plan if r["level"] == s}) for s in range(5)}
    assert chunks == {4: [(0, 160), (160, 160)], 3: [(0, 320)], 2: [(0, 320)], 1: [(0, 320)], 0: [(0, 320)]}
    done = collections.Counter()
    for r in plan:
        done[(r["level"], r["warp"], r["pair0"])] += r["K"]
    assert len(done) == 6 * 5 and set(done.values()) == {300}
    p = _ffi.default_tvl1_params(epsilon=0.0)
    assert _ffi.lib().va_tvl1_launch_plan(224, 224, 32, 11, ctypes.byref(p), None, None, 0) == len(plan)
    few = (_ffi.Tvl1Launch * 3)()
    assert _ffi.lib().va_tvl1_launch_plan(224, 224, 32, 11, ctypes.byref(p), None, few, 3) == len(plan)
    assert [(r.level, r.K, r.it0) for r in few] == [(r["level"], r["K"], r["it0"]) for r in plan[:3]]
    with pytest.raises(ValueError, match="out of range"):
        vflow.launch_plan(8, 8, 1, 2)
    with pytest.raises(ValueError, match=r"retired.*Valid stream_waves: 0, 1, 2, 7, 8, 9"):
        vflow.launch_plan(224, 224, 1, 2, epsilon=0.0, stream_waves=4)


# ---------------------------------------------------------------------------------------------------- GPU ----

_frames_cache = {}


def _frames(case):
    from video_analytics_amd import synth
    key = (case["S"], case["F"], case["H"], case["W"])
    if key not in _frames_cache:
        _, gray, _ = synth.synth_clips(case["S"], seed=7 * case["W"] + case["H"], H=case["H"], W=case["W"], n_gray=case["F"])
        _frames_cache[key] = gray
    return _frames_cache[key]


_oracle_cache = {}


def _oracle(oracle_tvl1, case):
    """The oracle's flow of a case: computed once per (frames, oracle parameters), shared and left unchanged."""
    kw = case["kw"]
    okw = {("lambda_" if k == "lambda" else k): v for k, v in kw.items() if k not in PRODUCT_ONLY}
    key = (case["S"], case["F"], case["H"], case["W"], tuple(sorted(okw.items())), kw.get("median", 0), kw.get("median_every", 0))
    if key not in _oracle_cache:
        gray = _frames(case).numpy()
        if kw.get("median", 0):
            import tvl1_median_oracle as mo
            ref = mo.tvl1_flow(gray, oracle_tvl1.default_params(**okw), kw["median"], kw.get("median_every", 0), nthreads=8)
        else:
            ref = oracle_tvl1.tvl1_flow(gray, oracle_tvl1.default_params(**okw), nthreads=8)
        ref.setflags(write=False)
        _oracle_cache[key] = ref
    return _oracle_cache[key]


def _run_counted(case):
    """tvl1_flow of a case with the launch counters on -> (flow on the host, launches per level the library counted)."""
    from video_analytics_amd import flow as vflow
    gray = _frames(case).cuda()
    vflow.profile_enable(True)
    try:
        vflow.profile_read(reset=True)
        vflow.profile_levels(16, reset=True)
        out = vflow.tvl1_flow(gray, **case["kw"])
        torch.cuda.synchronize()
        vflow.profile_read(reset=False)
        counted = [int(l["launches"]) for l in vflow.profile_levels(16, reset=True)]
        vflow.profile_read(reset=True)
    finally:
        vflow.profile_enable(False)
    return out.cpu().numpy(), counted


def _check_launches(cid, case):
    plan = _plan(case)
    props = _properties(plan, case["F"])
    assert set(case["must"]) <= props, (cid, sorted(set(case["must"]) - props))
    out, counted = _run_counted(case)
    want = [0] * 16
    for r in plan:
        if r["family"] != "median":
            want[r["level"]] += 1
    assert counted == want, (cid, counted, want)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cid", sorted(CASES))
def test_case_runs_the_launches_it_names_and_is_bit_exact(oracle_tvl1, cid):
    case = CASES[cid]
    out = _check_launches(cid, case)
    ref = _oracle(oracle_tvl1, case)
    assert out.shape == ref.shape == (case["S"] * (case["F"] - 1), 2, case["H"], case["W"])
    bad = np.flatnonzero((out != ref).reshape(len(out), -1).any(1))
    assert bad.size == 0, "%s: pairs %s differ, max abs diff %g" % (cid, bad[:8].tolist(), np.abs(out - ref).max())


_fast_group = {}


@pytest.mark.gpu
@pytest.mark.parametrize("cid", sorted(FAST_CASES))
def test_fast_math_case_runs_the_launches_it_names(oracle_tvl1, cid):
    """fast_math = 1: the 1-ulp arithmetic is the same in every kernel form, so the cases of a group (one frame and schedule)
    agree bit for bit -- the eight forced candidates with the stopping rule with each other, the five row pipelines with the
    register tiles --; in fixed-iteration mode the result stays within FAST_BOUND of the exact one (the oracle)."""
    case = FAST_CASES[cid]
    out = _check_launches(cid, case)
    assert np.isfinite(out).all()
    first = _fast_group.setdefault(case["group"], (cid, out))
    assert np.array_equal(out, first[1]), "%s differs from %s: max abs diff %g" % (cid, first[0], np.abs(out - first[1]).max())
    if case["kw"]["epsilon"] == 0.0:
        ref = _oracle(oracle_tvl1, case)
        d = np.abs(out - ref).max()
        assert 0.0 < d < FAST_BOUND, (cid, d)
