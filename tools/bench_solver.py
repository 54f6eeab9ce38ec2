"""Timings of the solver: weight decay, the dropout ratio and frozen layers in the fused training step.
Prints one JSON line per measurement.

    python tools/bench_solver.py variants [--batch 32] [--reps 5]
    python tools/bench_solver.py step     [--batch 32] [--reps 5] [--root DIR]
    python tools/bench_solver.py ab --parent DIR [--runs 3]

``variants``: per stream (c_in 3 and 20), the fused step under the default solver, ``weight_decay=5e-4``, ``dropout=0.8`` and
``freeze`` in {5, 10, 13, 16}, ``train_apply`` with and without decay, and the inference forward pass at the same batch
(what ``freeze=13`` approaches from above, together with the classifier backward), all interleaved in one process; HIP-event
time per call, median over the repetitions.
``step``: the step of a model whose solver was never set, per stream: the one measurement that also runs on a checkout without
the solver.  ``--root DIR`` takes the package from that checkout (built there) instead of this one.
``ab``: ``step`` on this checkout and on the parent's in alternating fresh processes, ``--runs`` each; the pair swaps its
order from run to run, so that neither side always follows the other.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _interleaved(runs, warmup, reps):
    ms = dict((k, []) for k in runs)
    for i in range(warmup + reps):
        for k, fn in runs.items():
            dt = _event_ms(lambda: fn(i))
            if i >= warmup:
                ms[k].append(dt)
    return ms


def _row(ms, **head):
    row = dict(head)
    for k, v in ms.items():
        row.update({k + "_ms": round(statistics.median(v), 4), k + "_ms_min": round(min(v), 4), k + "_ms_max": round(max(v), 4)})
    return row


def _streams(batch):
    import torch
    from video_analytics_amd import pipeline, vgg
    from video_analytics_amd.parameters import NACTION_CLASSES, VIDEO_DESCRIPTOR_DIM, VIDEO_INPUT_FLOW_COUNT as L
    dev = torch.device("cuda", 0)
    for c_in, name in ((3, "spatial"), (2 * L, "temporal")):
        w = pipeline.build_stream_weights(c_in, 1, dev)
        m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], NACTION_CLASSES, VIDEO_DESCRIPTOR_DIM)
        g = torch.Generator(device=dev).manual_seed(c_in)
        x = torch.randn((batch, c_in, 224, 224), generator=g, device=dev)
        y = (torch.arange(batch, device=dev) % NACTION_CLASSES).long()
        yield name, c_in, m, x, y
        m.close()


def variants(args):
    from video_analytics_amd import vgg
    S = vgg.Solver
    solvers = dict(default=S(), decay=S(weight_decay=5e-4), dropout08=S(dropout=0.8), freeze5=S(freeze=5), freeze10=S(freeze=10),
                   freeze13=S(freeze=13), freeze16=S(freeze=16))
    for name, c_in, m, x, y in _streams(args.batch):
        m.train_accumulate(x, y, first=True, dropout_seed=0)  # a gradient for the two apply forms

        def fused(sv, i):
            m.set_solver(sv)
            m.train_step(x, y, 0.0, 0.9, i)  # lr = 0 keeps the weights where they are

        def apply(sv):
            m.set_solver(sv)
            m.train_apply(0.0, 0.9)

        runs = dict(("step_" + k, (lambda sv: lambda i: fused(sv, i))(sv)) for k, sv in solvers.items())
        runs["apply"] = lambda i: apply(solvers["default"])
        runs["apply_decay"] = lambda i: apply(solvers["decay"])
        runs["forward"] = lambda i: m.forward(x)
        ms = _interleaved(runs, args.warmup, args.reps)
        print(json.dumps(_row(ms, metric="solver_step_ms", stream=name, c_in=c_in, batch=args.batch, reps=args.reps)), flush=True)


def step(args):
    for name, c_in, m, x, y in _streams(args.batch):
        ms = _interleaved(dict(step=lambda i: m.train_step(x, y, 0.0, 0.9, i)), args.warmup, args.reps)
        print(json.dumps(_row(ms, metric="default_step_ms", root=os.path.abspath(args.root), stream=name, c_in=c_in, batch=args.batch,
                              reps=args.reps)), flush=True)


def ab(args):
    if not args.parent or not os.path.exists(os.path.join(args.parent, "video_analytics_amd", "libva_hip.so")):
        sys.stderr.write("bench_solver.py ab: --parent must name a built checkout of the parent commit\n")
        sys.exit(2)
    for r in range(args.runs):
        for root in ((args.parent, HERE) if r % 2 == 0 else (HERE, args.parent)):  # alternating fresh processes
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "step", "--root", root, "--batch", str(args.batch),
                                   "--reps", str(args.reps), "--warmup", str(args.warmup)], timeout=300)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["variants", "step", "ab"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    if args.mode == "ab":
        return ab(args)
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_solver.py: no GPU visible; the hot path has no CPU fallback\n")
        sys.exit(2)
    torch.cuda.set_device(0)
    dict(variants=variants, step=step)[args.mode](args)


if __name__ == "__main__":
    main()
