"""One rank of tests/test_accum_gpu.py::test_two_ranks_agree_with_one_process (not a test module): started twice by
``launch.spawn_ranks`` with VA_DIST_BACKEND=gloo and VA_FORCE_DEVICE=0.  Exits non-zero on the first difference."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402
import torch.distributed as tdist  # noqa: E402

from video_analytics_amd import _ffi, augment, dist as vdist, pipeline, synth, vgg  # noqa: E402

LR, MU, CLIP = 1e-4, 0.9, 0.05
KEYS = ("conv_w", "conv_b", "fc_w", "fc_b")


def state(m):
    st, mo = m.export_state(), m.export_state(momentum=True)
    return [t for d in (st, mo) for k in KEYS for t in d[k]]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(a, b))


def digest(tensors):
    """Two int64 checksums of every tensor's bits: what the ranks exchange in place of a gigabyte of state."""
    rows = []
    for t in tensors:
        b = t.contiguous().view(torch.int32).view(-1).to(torch.int64)
        i = torch.arange(b.numel(), device=b.device, dtype=torch.int64) % 65521 + 1
        rows.append([int(b.sum()), int((b * i).sum())])
    return torch.tensor(rows, dtype=torch.int64)


def ranks_agree(tensors, what):
    mine = digest(tensors)
    both = [torch.zeros_like(mine) for _ in range(2)]
    tdist.all_gather(both, mine)
    if not torch.equal(both[0], both[1]):
        sys.exit("%s: the two ranks' states differ" % what)


def main():
    rank, _, world = vdist.init()
    assert world == 2, world
    device = int(os.environ["VA_FORCE_DEVICE"])
    torch.cuda.set_device(device)

    # ---- stream level ----
    w = synth.synth_vgg16_weights(c_in=3, seed=4)
    xs = [torch.from_numpy(synth.hash_uniform(95 + j, 3, 2 * 3 * 224 * 224).reshape(2, 3, 224, 224) * 4.0 - 2.0).cuda() for j in range(2)]
    ys = [torch.tensor([4, 9]).cuda(), torch.tensor([0, 100]).cuda()]
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256)
    m.train_accumulate(xs[rank], ys[rank], scales=0.5, first=True, dropout_seed=2000 + rank)
    vdist.all_reduce_gradients(m.grad())
    norm = m.train_apply(LR, MU, CLIP)
    got = state(m)
    ranks_agree(got, "stream level")
    if rank == 0:
        one = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256)
        for j in range(2):
            one.train_accumulate(xs[j], ys[j], scales=0.5, first=(j == 0), dropout_seed=2000 + j)
        norm1 = one.train_apply(LR, MU, CLIP)
        if not (float(norm) > CLIP and torch.equal(norm, norm1) and same(got, state(one))):
            sys.exit("stream level: two ranks differ from one process (norms %r %r)" % (float(norm), float(norm1)))
        one.close()
    m.close()
    del got

    # ---- pipeline level: one video per rank against micro_videos=1 on both videos ----
    from test_video_gpu import SCHEDULE, _synthetic_video
    vids = [tuple(t.cuda() for t in _synthetic_video(25, 240, 320, seed=s)) for s in (61, 63)]
    starts = [[0, 14], [3, 12]]
    crops = augment.draw_scale_jitter_crops(4, 240, 320, random.Random(3))
    labels = torch.tensor([50, 77])
    kw = dict(device=device, tvl1_params=_ffi.default_tvl1_params(**SCHEDULE))
    args = dict(k=2, lr=LR, momentum=MU, dropout_seed=5, clip_norm=CLIP)
    pipe = pipeline.TwoStreamPipeline(**kw)
    out = pipe.train_videos(vids[rank:rank + 1], labels[rank:rank + 1], starts=starts[rank:rank + 1], crops=crops[2 * rank:2 * rank + 2],
                            micro_videos=1, data_parallel=True, **args)
    got = state(pipe.spatial) + state(pipe.temporal)
    ranks_agree(got + [out["stats_s"], out["stats_t"]], "pipeline level")
    if rank == 0:
        one = pipeline.TwoStreamPipeline(**kw)
        ref = one.train_videos(vids, labels, starts=starts, crops=crops, micro_videos=1, **args)
        ok = same(got, state(one.spatial) + state(one.temporal))
        ok = ok and all(same([out[k]], [ref[k]]) for k in ("stats_s", "stats_t")) and all(torch.equal(out[k], ref[k]) for k in ("norm_s", "norm_t"))
        ok = ok and same([out["desc_s"], out["desc_t"]], [ref["desc_s"][:2], ref["desc_t"][:2]])
        if not ok:
            sys.exit("pipeline level: data_parallel=True on two ranks differs from micro_videos=1 in one process")
        one.close()
    pipe.close()
    vdist.barrier()
    tdist.destroy_process_group()


if __name__ == "__main__":
    main()
