"""The stream choreography of ``TwoStreamPipeline`` without a GPU: every operation the pipeline puts on a stream -- event
records and waits, stream waits, ``record_stream`` calls, TV-L1 calls, model forwards and the device wrappers with the
pipeline buffer they write -- is recorded in order and compared with ``tests/golden/pipeline_stream_trace.json``.

A dropped or moved ``wait_event`` is a race that the bit-for-bit GPU tests rarely see on a quiet machine; here it is a changed
line.  The golden is written by ``tests/golden/make_pipeline_stream_trace.py`` with the recorder below.

Streams are named ``caller`` (the current stream outside any ``torch.cuda.stream`` block), ``cnn`` and ``cnn2`` (the two
streams the constructor creates, in that order) and ``flow0...``; events are numbered in creation order.  Tensors appear as
their shape, prefixed with bank and slot where their storage is one of the pipeline's own buffers (``flow[0]:20x2x224x224``).
"""
import contextlib
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_stream_trace.json")
DEV = torch.device("cuda", 0)
BANKS = ("_flow", "_stack", "_motion", "_dstack")  # the pipeline's cross-stream buffers, ``depth`` slots each
L = 10


class OnDevice(torch.Tensor):
    """A host tensor that says it lives on the pipeline's device: the host checks pass and no GPU is needed."""
    is_cuda = property(lambda self: True)
    device = property(lambda self: DEV)


def dev(t):
    return t.as_subclass(OnDevice)


class Recorder(object):
    def __init__(self):
        self.trace, self.pipe = [], None
        self.n_events = self.n_streams = 0
        self.current = ["caller"]
        self.flow_streams = {}

    def log(self, *entry):
        self.trace.append(list(entry))

    def desc(self, t):
        if t is None:
            return None
        if isinstance(t, (list, tuple)):
            return [self.desc(x) for x in t]
        shape = "x".join(str(int(d)) for d in t.shape)
        for bank in BANKS if self.pipe is not None else ():
            for k, b in enumerate(getattr(self.pipe, bank)):
                if b is not None and b.untyped_storage().data_ptr() == t.untyped_storage().data_ptr():
                    return "%s[%d]:%s" % (bank[1:], k, shape)
        return shape


def install(monkeypatch):
    """Replace streams, events, TV-L1, the models and the device wrappers with recorders -> the Recorder."""
    from video_analytics_amd import augment, flow, fusion, rgbdiff, vgg
    rec = Recorder()

    class Stream(object):
        def __init__(self, device=None, priority=0, name=None):
            if name is None:
                name = ("cnn", "cnn2")[rec.n_streams] if rec.n_streams < 2 else "stream%d" % rec.n_streams
                rec.n_streams += 1
            self.name = name

        def wait_event(self, ev):
            rec.log("wait_event", self.name, ev.id)

        def wait_stream(self, other):
            rec.log("wait_stream", self.name, other.name)

        def synchronize(self):
            rec.log("synchronize", self.name)

    class Event(object):
        def __init__(self, *a, **k):
            self.id = rec.n_events
            rec.n_events += 1

        def record(self, stream=None):
            rec.log("record", stream.name if stream is not None else rec.current[-1], self.id)

        def query(self):
            return True

        def synchronize(self):
            rec.log("event_synchronize", self.id)

    caller = Stream(name="caller")
    by_name = {"caller": caller}

    def make_stream(*a, **k):
        s = Stream(*a, **k)
        by_name[s.name] = s
        return s

    @contextlib.contextmanager
    def stream(s):
        rec.current.append(s.name)
        try:
            yield
        finally:
            rec.current.pop()

    def flow_streams(device, n):
        if n not in rec.flow_streams:
            rec.flow_streams[n] = [Stream(name="flow%d" % i) for i in range(n)]
        return rec.flow_streams[n]

    def tvl1_flow_concurrent(frames, params=None, n_streams=2, out=None, after=None, join=True):
        S, F, H, W = frames.shape
        if out is None:
            out = torch.empty((S * (F - 1), 2, H, W), dtype=torch.float32)
        cur = by_name[rec.current[-1]]
        rec.log("tvl1_flow_concurrent", cur.name, rec.desc(frames), rec.desc(out), "join" if join else "no join")
        streams = flow.flow_streams(frames.device, max(1, min(int(n_streams), S)))
        events = []
        for st in streams:
            if after is None:
                st.wait_stream(cur)
            for ev in (after if isinstance(after, (list, tuple)) else [after]):
                if ev is not None:
                    st.wait_event(ev)
            rec.log("tvl1", st.name)
            if not join:
                events.append(Event())
                events[-1].record(st)
        if not join:
            return out, events
        for st in streams:
            cur.wait_stream(st)
        return out

    view_chunk = vgg.Vgg16Stream.VIEW_CHUNK

    class Model(object):
        VIEW_CHUNK = view_chunk

        def __init__(self, conv_w, conv_b, fc_w, fc_b, n_classes, desc_dim, *norm, device=None, ws_slot=0, dtype="f32"):
            self.name = {1: "spatial", 0: "temporal", 2: "diff"}[ws_slot]
            self.n_classes, self.desc_dim, self.dtype = n_classes, desc_dim, dtype

        def forward(self, x):
            rec.log("forward", self.name, rec.current[-1], rec.desc(x))
            B = x.shape[0]
            return None, torch.zeros(B, self.desc_dim), torch.zeros(B, self.n_classes)

        def forward_views(self, x):
            rec.log("forward_views", self.name, rec.current[-1], rec.desc(x))
            B, V = x.shape[:2]
            return (torch.zeros(B, self.desc_dim), torch.zeros(B, self.n_classes), torch.zeros(B, V, self.desc_dim),
                    torch.zeros(B, V, self.n_classes))

        def train_step_consensus(self, x, labels, k, lr, momentum, dropout_seed):
            rec.log("train_step_consensus", self.name, rec.current[-1], rec.desc(x))
            return torch.zeros(2), torch.zeros(x.shape[0], self.desc_dim)

        def close(self):
            rec.log("close", self.name)

    def wrapper(name, result):
        """A device wrapper: logs name, current stream, first argument and ``out=``; returns ``out`` or ``result(...)``."""
        def call(x, *a, **k):
            out = k.get("out")
            rec.log(name, rec.current[-1], rec.desc(x), rec.desc(out))
            return out if out is not None else result(x, *a, **k)
        return call

    def apply_camera(fl, camera="none", in_place=False):
        rec.log("apply_camera", rec.current[-1], rec.desc(fl), camera, bool(in_place))
        if camera == "none":
            return fl, None, None
        return fl, torch.zeros(fl.shape[0], 3, 3, dtype=torch.float64), torch.zeros(fl.shape[0], dtype=torch.float64)

    def fuse(scores, *a, **k):
        first = scores[0] if isinstance(scores, (list, tuple)) else scores
        return torch.zeros(tuple(first.shape)), torch.zeros(first.shape[0], dtype=torch.int32)

    def images(x, table, *a, **k):  # [n,c,h,w], one row per output image -> u8 [rows,c,224,224]
        return torch.empty((table.shape[0], x.shape[1], 224, 224), dtype=torch.uint8)

    wrappers = {
        flow: dict(
            flow_to_stack=lambda fl, **k: torch.empty((2 * fl.shape[0],) + tuple(fl.shape[2:])),
            crop_flow_to_stack=None, crop_flow_to_stack_views=None, crop_flow_to_stack_snippets=None,
            flowq_to_stack_snippets=None,
            apply_motion=lambda fl, *a, **k: fl,
            resize_flow_to_stack=lambda fl, table, **k: torch.empty((table.shape[0], 224, 224))),
        augment: dict(
            crop_images=lambda x, crops, **k: torch.empty((x.shape[0], x.shape[1], 224, 224), dtype=torch.uint8),
            crop_image_views=lambda x, views, **k: torch.empty((x.shape[0], views.shape[0], x.shape[1], 224, 224),
                                                               dtype=torch.uint8),
            crops_to_device=lambda t, device: t,
            resize_images=images),
        rgbdiff: dict(rgb_diff_stack=lambda x, table, n_diff, **k: torch.empty((table.shape[0], 3 * n_diff, 224, 224))),
        fusion: dict(score_consensus=lambda lg, mode="softmax": torch.zeros(lg.shape[0], lg.shape[-1]),
                     fuse_scores=fuse, fuse_scores_n=fuse),
        vgg: dict(view_mean=lambda x: torch.zeros((x.shape[0],) + tuple(x.shape[2:]))),
    }
    for mod, table in wrappers.items():
        for name, result in table.items():
            monkeypatch.setattr(mod, name, wrapper(name, result))
    monkeypatch.setattr(flow, "apply_camera", apply_camera)
    monkeypatch.setattr(flow, "flow_streams", flow_streams)
    monkeypatch.setattr(flow, "tvl1_flow_concurrent", tvl1_flow_concurrent)
    monkeypatch.setattr(vgg, "Vgg16Stream", Model)
    monkeypatch.setattr(torch.cuda, "Stream", make_stream)
    monkeypatch.setattr(torch.cuda, "Event", Event)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: by_name[rec.current[-1]])
    monkeypatch.setattr(torch.cuda, "stream", stream)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.Tensor, "record_stream",
                        lambda t, s: rec.log("record_stream", rec.current[-1], rec.desc(t), s.name))
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **k: real_empty(*a, **k))  # the pipeline's buffers: on the host
    return rec


def make_pipe(rec, **kw):
    """A pipeline through its own constructor (the recorders stand in for the streams and the models)."""
    from video_analytics_amd import pipeline
    w = dict(conv_w=None, conv_b=None, fc_w=None, fc_b=None)
    rec.pipe = pipeline.TwoStreamPipeline(device=0, weights=[w] * (3 if kw.get("rgb_diff") else 2), flow_count=L, **kw)
    return rec.pipe


def batch(B=2, H=224, W=224):
    return dev(torch.zeros(B, 3, H, W, dtype=torch.uint8)), dev(torch.zeros(B, L + 1, H, W, dtype=torch.uint8))


def clip(T=20, H=224, W=224):
    return dev(torch.zeros(T, 3, H, W, dtype=torch.uint8)), dev(torch.zeros(T, H, W, dtype=torch.uint8))


# ---- the scenarios: each runs on a fresh recorder and a fresh pipeline ----

def s1_three_submits_depth2(rec):
    pipe = make_pipe(rec)
    for _ in range(3):  # the third reuses slot 0 and waits for its flow-read event
        pipe.submit(*batch())
    pipe.wait()


def s1_three_submits_depth1_one_flow_stream(rec):
    pipe = make_pipe(rec, depth=1, flow_streams=1)
    for _ in range(3):
        pipe.submit(*batch())
    pipe.wait()


def s2_flow_stack_then_live(rec):
    pipe = make_pipe(rec)
    rgb, gray = batch()
    for _ in range(2):  # the temporal-done event crosses between cnn2 and cnn
        pipe.submit(rgb, flow_stack=dev(torch.zeros(2, 2 * L, 224, 224)))
    pipe.submit(rgb, gray)
    pipe.wait()


def s3_crops_camera_mean_flow(rec):
    from video_analytics_amd import augment
    import random
    pipe = make_pipe(rec, camera="homography", mean_flow=True)
    rgb, gray = batch(2, 240, 320)
    crops = augment.draw_clip_crops(2, L, (240, 320), (240, 320), rng=random.Random(3))
    for _ in range(2):
        pipe.submit(rgb, gray, crops=crops, invert_flow_x=True)
    pipe.wait()


def s4_views_trajectory_then_another_size(rec):
    from video_analytics_amd import augment
    pipe = make_pipe(rec, motion="trajectory")
    v = augment.ten_crop_views(240, 320)
    for _ in range(2):
        pipe.submit(*batch(2, 240, 320), views=(v, v))
    pipe.submit(*batch(1, 240, 320), views=(v, v))  # slot 0 again: its buffers are dropped, one retire event per stream
    pipe.wait()


def s5_video_live_ten_crop(rec):
    from video_analytics_amd import augment
    pipe = make_pipe(rec)
    v = augment.ten_crop_views(240, 320)
    for _ in range(2):
        pipe.submit_video(*clip(20, 240, 320), n_snippets=3, views=(v, v))
    pipe.wait()


def s5_video_rgb_diff(rec):
    from video_analytics_amd import augment
    pipe = make_pipe(rec, rgb_diff=True)
    v = augment.ten_crop_views(240, 320)
    pipe.submit_video(*clip(20, 240, 320), n_snippets=3, views=(v, v), fusion_weights=(1.0, 1.5, 0.5))
    pipe.wait()


def s5_video_stored_f32_mean_flow(rec):
    pipe = make_pipe(rec, mean_flow=True)
    pipe.submit_video(clip()[0], None, n_snippets=3, flow=dev(torch.zeros(19, 2, 224, 224)))
    pipe.wait()


def s5_video_stored_u8(rec):
    pipe = make_pipe(rec)
    pipe.submit_video(clip()[0], None, n_snippets=3, flow=dev(torch.zeros(19, 2, 224, 224, dtype=torch.uint8)))
    pipe.wait()


def s6_mixed_paths(rec):
    pipe = make_pipe(rec)
    rgb, gray = batch()
    pipe.submit(rgb, gray)
    pipe.submit_video(*clip(), n_snippets=3)
    pipe.submit(rgb, flow_stack=dev(torch.zeros(2, 2 * L, 224, 224)))
    pipe.wait()
    pipe.close()


def s7_train_between_submits(rec):
    pipe = make_pipe(rec)
    pipe.submit(*batch())
    crops = torch.tensor([[0, 0, 224, 224, 0], [0, 0, 224, 224, 1]], dtype=torch.int32)
    pipe.train_videos([clip(), clip()], [3, 4], k=1, starts=[[2], [5]], crops=crops)
    pipe.submit(*batch())
    pipe.wait()


SCENARIOS = (s1_three_submits_depth2, s1_three_submits_depth1_one_flow_stream, s2_flow_stack_then_live,
             s3_crops_camera_mean_flow, s4_views_trajectory_then_another_size, s5_video_live_ten_crop, s5_video_rgb_diff,
             s5_video_stored_f32_mean_flow, s5_video_stored_u8, s6_mixed_paths, s7_train_between_submits)


def record(scenario):
    """-> the trace of one scenario; everything replaced is restored before this returns."""
    with pytest.MonkeyPatch.context() as mp:
        rec = install(mp)
        scenario(rec)
    return rec.trace


def render(traces):
    """{scenario: trace} -> the golden file's text: one operation per line."""
    parts = []
    for name, trace in traces.items():
        parts.append("%s: [\n%s\n]" % (json.dumps(name), ",\n".join("  " + json.dumps(e) for e in trace)))
    return "{\n%s\n}\n" % ",\n".join(parts)


def test_every_scenario_has_a_golden_trace():
    with open(GOLDEN) as f:
        assert sorted(json.load(f)) == sorted(s.__name__ for s in SCENARIOS)


@pytest.mark.parametrize("scenario", SCENARIOS, ids=[s.__name__ for s in SCENARIOS])
def test_stream_operations_keep_their_order(scenario):
    with open(GOLDEN) as f:
        want = json.load(f)[scenario.__name__]
    got = record(scenario)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "operation %d: got %r, the golden has %r (after %r)" % (i, g, w, got[max(0, i - 3):i])
    assert len(got) == len(want), "%d operations, the golden has %d; the first extra one: %r" % (
        len(got), len(want), (got + want)[min(len(got), len(want))])


def test_the_golden_file_is_what_the_recorder_writes():
    """Byte for byte: the file is ``render`` of the traces, so ``make_pipeline_stream_trace.py`` would rewrite it unchanged."""
    with open(GOLDEN) as f:
        assert f.read() == render({s.__name__: record(s) for s in SCENARIOS})
