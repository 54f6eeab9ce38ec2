"""The cost of HMM action segmentation on one MI355X, at a Breakfast-like load.  One JSON line per
measurement.

    python tools/bench_hmm.py [--videos 100] [--frames 2000] [--reps 5] [--warmup 1] [--host]

100 videos x 2,000 frames x 64 columns; 48 units of 8 states (G = 384); 50 grammars of 6 units (N = 48 states a model).

  emissions_ms       ``va_hmm_emissions`` over all frames: logB [200,000, 384]
  score_all_ms       ``va_hmm_viterbi`` over all 5,000 (video, grammar) pairs without backpointers (the single-wave form)
  decode_best_ms     the 100 winners again, with backpointers and the backtrack
  segment_ms         ``hmm.segment`` whole: compose, emissions, both Viterbi passes and the host's part
  score_sweep_ms     the score pass on 256, 1,024, 4,096, 8,192 and 16,384 jobs (1 to 64 chains offered per CU): flat where a
                     chain waits on its own steps, proportional where the CU is full.  Each row carries the achieved share of
                     the ceiling the sweep gives (``share_of_ceiling``): 256 CUs x the chains a CU holds, each finishing a
                     step per step latency, the latency taken from the least time of the 256-job row;
                     ``score_all_share`` is that share for the load's own 5,000 jobs
  fb_ms              ``va_hmm_forward_backward`` over 500 unit sequences of 400 frames under their units' models (N = 8)
  fit_iter_ms        one Baum-Welch iteration of ``hmm.fit`` over those sequences: emissions, forward-backward, statistics, M-step
  wg_score_ms, wg_decode_ms, wg_fb_ms   the same kernels at N = 1024 (left-to-right, the workgroup form)

HIP events around each call, median of --reps with the range; the calls of one group are interleaved (one of each per round).
The times are those of the Python calls: they hold the packing of the models, the launches and the copies of the results
back.  Beside each time stand frames x edges per second (one add and one compare per frame and edge), the bytes of logB the
chains read per second next to the HBM peak (8 TB/s; every byte counted although the grammars of one video share its rows in
cache), and ``step_ns``: the time over the frames of the jobs that one CU's resident chains run one after another
(``chains_per_cu`` from the kernel's LDS and the 32 waves of a CU), which is the latency of one dependent step of the chain.
Which of the three a pass obeys is read from those figures; the tool states none of them in advance.

--host adds the numpy restatement (tests/hmm_oracle.py) on the host for ONE (video, grammar) pair, one run: a figure to set
the scale, not a race.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_TBS, CUS, LDS_PER_CU, WAVES_PER_CU = 8.0, 256, 160 * 1024, 32


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def interleaved(variants, warmup, reps):
    """{name: [ms]}: one call of each variant per round"""
    out = {name: [] for name in variants}
    for r in range(warmup + reps):
        for name, fn in variants.items():
            ms = timed(fn)[1]
            if r >= warmup:
                out[name].append(ms)
    return out


def kernel_lds():
    """{kernel name: (LDS bytes, workgroup size)} of the hmm kernels, from the library's own metadata."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    return {r["name"]: (r["lds"], r["max_wg"]) for r in kernel_resources.kernels() if "k_hmm" in r["name"]}


def chains_per_cu(lds, kernel):
    """The workgroups of ``kernel`` one CU holds: its LDS against 160 KB, its waves against 32."""
    nbytes, wg = lds[kernel]
    return max(1, min(LDS_PER_CU // max(nbytes, 1), WAVES_PER_CU // (wg // 64)))


def report(metric, ms, jobs=0, frames=0, edges=0, states=0, per_cu=0, **more):
    med = statistics.median(ms)
    row = dict(metric=metric, ms=round(med, 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3), reps=len(ms))
    if jobs:
        waves = -(-jobs // (CUS * per_cu))  # how many chains one slot of a CU runs one after another
        row.update(jobs=jobs, frames_per_job=frames, edges_per_model=edges, states_per_model=states,
                   frame_edges_per_s=round(jobs * frames * edges / med * 1e3, 1),
                   logb_tb_per_s=round(jobs * frames * states * 8.0 / med / 1e9, 4), hbm_peak_tb_per_s=HBM_PEAK_TBS,
                   chains_per_cu=per_cu, step_ns=round(med * 1e6 / (waves * frames), 1))
    row.update(more)
    print(json.dumps(row), flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=100)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from video_analytics_amd import hmm
    if not torch.cuda.is_available():
        raise RuntimeError("bench_hmm.py measures on an MI355X: torch.cuda.is_available() is False")
    dev = torch.device("cuda", 0)
    lds = kernel_lds()
    rng = np.random.RandomState(0)
    nv, T, D, nu, ns, ng, gl = args.videos, args.frames, 64, 48, 8, 50, 6
    G = nu * ns
    hs = hmm.HmmSet(rng.randn(G, D), rng.uniform(0.5, 2.0, (G, D)))
    names = ["u%02d" % u for u in range(nu)]
    for u, nm in enumerate(names):
        hs.add_unit(hmm.HmmSet.left_to_right(nm, u * ns, ns))
    grammars = [[names[i] for i in rng.randint(0, nu, gl)] for _ in range(ng)]
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((nv * T, D), generator=gen, device=dev, dtype=torch.float32)
    seg = np.arange(nv + 1, dtype=np.int64) * T
    models = [hs.compose(g) for g in grammars]
    N, E = models[0].n_states, models[0].n_edges
    logb = hmm.emissions(x, hs)
    pairs = np.array([(v, g, 0) for v in range(nv) for g in range(ng)], dtype=np.int32)
    scores = hmm.viterbi(logb, models, pairs, segments=seg)[0].reshape(nv, ng)
    winners = np.array([(v, g, 1) for v, g in enumerate(hmm.best_grammar(scores))], dtype=np.int32)

    t = interleaved({"emissions": lambda: hmm.emissions(x, hs), "score": lambda: hmm.viterbi(logb, models, pairs, segments=seg),
                     "decode": lambda: hmm.viterbi(logb, models, winners, segments=seg),
                     "segment": lambda: hmm.segment(x, hs, grammars, segments=seg)}, args.warmup, args.reps)
    med = statistics.median(t["emissions"])
    print(json.dumps(dict(metric="emissions_ms", ms=round(med, 3), ms_min=round(min(t["emissions"]), 3), ms_max=round(max(t["emissions"]), 3),
                          reps=len(t["emissions"]), frames=nv * T, d=D, g=G, f64_tflops=round(4.0 * nv * T * G * D / med / 1e9, 3),
                          tb_per_s=round((4.0 * nv * T * D + 8.0 * nv * T * G) / med / 1e9, 4), hbm_peak_tb_per_s=HBM_PEAK_TBS,
                          note="4 flops per frame, Gaussian and column on the vector unit; bytes: x read, logB written")), flush=True)
    wave = chains_per_cu(lds, "k_hmm_viterbi<64, 1>")
    score_med = report("score_all_ms", t["score"], len(pairs), T, E, N, wave)
    report("decode_best_ms", t["decode"], len(winners), T, E, N, wave, note="with uint16 backpointers [T, N] and the backtrack")
    report("segment_ms", t["segment"], note="hmm.segment whole: compose, emissions, score all pairs, decode the winners")

    # what the score pass is bound by: the same pairs, tiled to 1, 4, 16, 32 and 64 chains per CU.  Where the time does not
    # grow with the chains a CU holds at once, a chain waits on its own dependent steps (latency) and more chains are free;
    # where it grows in proportion, the CU's issue slots or LDS are full (throughput).
    sweep = {}
    for nj in (CUS, 4 * CUS, 16 * CUS, 32 * CUS, 64 * CUS):
        tiled = np.ascontiguousarray(np.tile(pairs, (-(-nj // len(pairs)), 1))[:nj])
        sweep[nj] = (lambda jobs=tiled: hmm.viterbi(logb, models, jobs, segments=seg))
    t = interleaved(sweep, args.warmup, args.reps)
    # the ceiling the sweep itself gives: every chain a CU can hold (``wave`` per CU) finishing one step per step latency, the
    # latency being the LEAST time of the one-chain-per-CU row over its frames (the least, because other work on the machine
    # only ever adds to a latency; the call's fixed cost is included, so it is still an upper bound)
    step_s = min(t[CUS]) * 1e-3 / T
    ceiling = CUS * wave * E / step_s
    for nj, ms in t.items():
        med = statistics.median(ms)
        rate = nj * T * E / med * 1e3
        print(json.dumps(dict(metric="score_sweep_ms", jobs=nj, chains_per_cu_offered=nj // CUS, ms=round(med, 3), ms_min=round(min(ms), 3),
                              ms_max=round(max(ms), 3), reps=len(ms), ns_per_frame_of_one_chain=round(med * 1e6 / T, 1),
                              frame_edges_per_s=round(rate, 1), chains_per_cu_resident=wave, step_latency_ns=round(step_s * 1e9, 1),
                              ceiling_frame_edges_per_s=round(ceiling, 1), share_of_ceiling=round(rate / ceiling, 3))), flush=True)
    rate = len(pairs) * T * E / score_med * 1e3
    print(json.dumps(dict(metric="score_all_share", jobs=len(pairs), frame_edges_per_s=round(rate, 1), ceiling_frame_edges_per_s=round(ceiling, 1),
                          share_of_ceiling=round(rate / ceiling, 3),
                          note="bound: step latency while a CU has free chain slots, then the chains a CU holds; the ceiling is both together")),
          flush=True)

    # one Baum-Welch iteration over 500 unit sequences
    n_seq, ts = 5 * nv, T // 5
    useg = np.arange(n_seq + 1, dtype=np.int64) * ts
    unit_of = [names[i % nu] for i in range(n_seq)]
    umodels = [hs.compose([nm]) for nm in names]
    ujobs = np.array([(i, i % nu, 0) for i in range(n_seq)], dtype=np.int32)
    t = interleaved({"fb": lambda: hmm.forward_backward(logb, umodels, ujobs, segments=useg),
                     "fit": lambda: hmm.fit(x, unit_of, ns, iters=1, segments=useg)}, args.warmup, args.reps)
    report("fb_ms", t["fb"], n_seq, ts, umodels[0].n_edges, ns, chains_per_cu(lds, "k_hmm_fb<64, 1>"),
           note="forward and backward: two dependent passes per frame; the call copies gamma [frames, 8] back to the host")
    report("fit_iter_ms", t["fit"], note="hmm.fit(iters=1) whole: the first alignment's statistics, emissions, forward-backward, "
                                         "statistics, M-step")

    # the workgroup form: N = 1024
    big_n, big_jobs = 1024, 256
    i = np.arange(big_n)
    la = np.where((i[:, None] == i[None, :]) | (i[:, None] + 1 == i[None, :]), np.log(0.5), -np.inf)
    big = hmm.Model.from_dense(la, np.log(np.full(big_n, 1.0 / big_n)), np.zeros(big_n), rng.randint(0, G, big_n))
    bjobs = np.array([(k % nv, 0, 0) for k in range(big_jobs)], dtype=np.int32)
    bdec = np.array([(k, 0, 1) for k in range(16)], dtype=np.int32)
    t = interleaved({"score": lambda: hmm.viterbi(logb, [big], bjobs, segments=seg), "decode": lambda: hmm.viterbi(logb, [big], bdec, segments=seg),
                     "fb": lambda: hmm.forward_backward(logb, [big], bdec[:8], segments=seg)}, args.warmup, args.reps)
    wg = chains_per_cu(lds, "k_hmm_viterbi<256, 4>")
    report("wg_score_ms", t["score"], big_jobs, T, big.n_edges, big_n, wg)
    report("wg_decode_ms", t["decode"], len(bdec), T, big.n_edges, big_n, wg)
    report("wg_fb_ms", t["fb"], 8, T, big.n_edges, big_n, chains_per_cu(lds, "k_hmm_fb<256, 4>"))

    if args.host:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import hmm_oracle
        m = models[0]
        dense = np.full((N, N), -np.inf)
        dense[m.pred_idx, np.repeat(np.arange(N), np.diff(m.pred_ptr))] = m.pred_logp
        rows = logb[:T].cpu().numpy()
        t0 = time.perf_counter()
        hmm_oracle.viterbi_fast(rows, m.emit, m.log_pi, dense, m.log_final)
        v = time.perf_counter() - t0
        t0 = time.perf_counter()
        hmm_oracle.forward_backward(rows, m.emit, m.log_pi, dense, m.log_final)
        print(json.dumps(dict(metric="host_numpy_one_pair", frames=T, states=N, viterbi_s=round(v, 4),
                              forward_backward_s=round(time.perf_counter() - t0, 4), threads=os.environ.get("OMP_NUM_THREADS"),
                              note="the numpy restatement on the host for ONE pair, one unrepeated run: scale, not a race")), flush=True)


if __name__ == "__main__":
    main()
