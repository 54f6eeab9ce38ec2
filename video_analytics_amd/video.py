"""Whole-video evaluation, host side: which snippets of a video are classified and which of its frame
pairs TV-L1 has to see for them.

The reference classifies clips; the papers it follows classify videos (Sheet03/notes.txt:113-116 and 225-230): 25 frames
or flow stacks with equal temporal spacing, ten crops of each, the class scores averaged, then the two streams fused
(notes.txt:121-124).  ``snippetStarts`` places the snippets, ``snippetPlan`` lists the frame pairs they share so that
each goes through TV-L1 once, and ``evaluateVideos`` is the loop over videos on ``TwoStreamPipeline.submit_video``.
Everything here but ``evaluateVideos`` is integer arithmetic on the host.

Training samples differently (TSN, notes.txt:165-175): ``segmentStarts`` draws one snippet from each of k
equal segments and ``segmentPlan`` lists the pairs those snippets need (``TwoStreamPipeline.train_videos``).
"""
import numpy as np

from .parameters import VIDEO_INPUT_FLOW_COUNT

N_SNIPPETS = 25  # both papers' testing protocol


def snippetStarts(T, L=VIDEO_INPUT_FLOW_COUNT, n=N_SNIPPETS):
    """The 0-based first frame pair of each of ``n`` snippets of a ``T``-frame video (pair p = frames p, p + 1; P = T - 1
    pairs), ``L`` pairs per snippet: ``s_i = (i * (P - L)) // (n - 1)``, equally spaced from the first window to the last;
    one snippet sits in the centre, ``(P - L) // 2``.  Snippet i covers pairs ``s_i .. s_i + L - 1`` and its RGB frame is
    frame ``s_i`` (the paper's volume I_tau starts at the sampled frame tau).  A short video gives duplicate starts; they
    are kept.  ValueError when the video holds no window (``P < L``) or ``n < 1``."""
    T, L, n = int(T), int(L), int(n)
    P = T - 1
    if L < 1:
        raise ValueError("snippetStarts: need at least one flow pair per snippet, got L=%d" % L)
    if n < 1:
        raise ValueError("snippetStarts: need at least one snippet, got n=%d" % n)
    if P < L:
        raise ValueError("snippetStarts: a video of %d frames has %d frame pairs, fewer than one snippet's %d" % (T, P, L))
    if n == 1:
        return [(P - L) // 2]
    return [(i * (P - L)) // (n - 1) for i in range(n)]


class SnippetPlan(object):
    """What ``snippetPlan`` returns.

      * ``starts``   the snippets' first pairs in the video (``snippetStarts``); also their RGB frames,
      * ``pairs``    U: the sorted, duplicate-free pairs some snippet needs,
      * ``index``    each snippet's start re-indexed into U: its window is ``pairs[index[i] : index[i] + L]``,
      * ``sequences``  the TV-L1 input as frame indices ``[S][F]``: one two-frame sequence per pair of U, in U's order, so
                     that the flow comes out as ``[len(U),2,H,W]`` in U's order and any number of streams can share the
                     sequences without padding,
      * ``pair_computations``  TV-L1 pair computations this plan causes (``len(pairs)``: no padding pairs)."""

    def __init__(self, T, L, n):
        self.T, self.L, self.n = int(T), int(L), int(n)
        self.starts = snippetStarts(T, L, n)
        need = sorted(set(p for s in self.starts for p in range(s, s + self.L)))
        where = dict((p, j) for j, p in enumerate(need))
        self.pairs = need
        self.index = [where[s] for s in self.starts]
        self.sequences = [(p, p + 1) for p in need]
        self.pair_computations = len(self.sequences)


def snippetPlan(T, L=VIDEO_INPUT_FLOW_COUNT, n=N_SNIPPETS):
    """The pairs of a ``T``-frame video its ``n`` snippets need, each once (``SnippetPlan``).  A window of L consecutive
    pairs is contiguous in the sorted set U, because every pair of it is in U; ``len(U) <= min(T - 1, n * L)``.  At L = 10,
    n = 25: 149 pairs for a 150-frame video (250 for 25 independent clips), 250 of 299 at T = 300."""
    return SnippetPlan(T, L, n)


N_SEGMENTS = 3  # TSN's number of segments


def segmentStarts(T, k=N_SEGMENTS, L=VIDEO_INPUT_FLOW_COUNT, rng=None):
    """Training-time temporal segment sampling: the first frame pair of each of ``k`` snippets of a ``T``-frame video
    (P = T - 1 pairs, window starts 0 .. P - L).  ``avg = (P - L + 1) // k``; with ``avg > 0`` snippet i starts at
    ``i * avg + rng.randrange(avg)``, one per segment; a video with fewer than k starts gets the sorted list of k draws
    of ``rng.randrange(P - L + 1)``; ValueError when it holds no window.  ``rng``: a ``random.Random`` (default: the
    global generator).  Snippet i covers pairs ``s_i .. s_i + L - 1`` and its RGB frame is frame ``s_i``."""
    import random
    rng = random if rng is None else rng
    T, k, L = int(T), int(k), int(L)
    P = T - 1
    if L < 1:
        raise ValueError("segmentStarts: need at least one flow pair per snippet, got L=%d" % L)
    if k < 1:
        raise ValueError("segmentStarts: need at least one segment, got k=%d" % k)
    if P < L:
        raise ValueError("segmentStarts: a video of %d frames has %d frame pairs, fewer than one snippet's %d" % (T, P, L))
    avg = (P - L + 1) // k
    if avg > 0:
        return [i * avg + rng.randrange(avg) for i in range(k)]
    return sorted(rng.randrange(P - L + 1) for _ in range(k))


class SegmentPlan(SnippetPlan):
    """``SnippetPlan`` for given starts: ``pairs`` the sorted, duplicate-free pairs the windows need, ``index`` each start
    re-indexed into them, ``sequences`` one two-frame TV-L1 sequence per pair."""

    def __init__(self, T, starts, L):
        self.T, self.L = int(T), int(L)
        self.starts = [int(s) for s in starts]
        self.n = len(self.starts)
        P = self.T - 1
        if self.L < 1 or self.n < 1:
            raise ValueError("segmentPlan: need at least one snippet of at least one pair")
        if any(s < 0 or s + self.L > P for s in self.starts):
            raise ValueError("segmentPlan: a window of %d pairs starting at %d..%d does not lie in the %d pairs of a "
                             "%d-frame video" % (self.L, min(self.starts), max(self.starts), P, self.T))
        need = sorted(set(p for s in self.starts for p in range(s, s + self.L)))
        where = dict((p, j) for j, p in enumerate(need))
        self.pairs = need
        self.index = [where[s] for s in self.starts]
        self.sequences = [(p, p + 1) for p in need]
        self.pair_computations = len(self.sequences)


def segmentPlan(T, starts, L=VIDEO_INPUT_FLOW_COUNT):
    """The pairs of a ``T``-frame video the snippets at ``starts`` need, each once (``SegmentPlan``): at most ``k * L``,
    30 TV-L1 pairs per video at k = 3, L = 10.  ValueError when a window leaves the video."""
    return SegmentPlan(T, starts, L)


def evaluateVideos(pipe, videos, labels, flows=None, **kw):
    """The test protocol over a list of videos: ``videos`` yields ``(rgb u8 [T,3,H,W], gray [T,H,W])`` pairs on the
    pipeline's device, ``labels`` their class indices; ``kw`` goes to ``TwoStreamPipeline.submit_video``.  Returns
    ``(acc_spatial, acc_temporal, acc_fused, descriptors)``: the fractions of videos whose spatial, temporal and fused
    scores have their first maximum at the label, and the float32 ``[N,512]`` joined descriptors (spatial then temporal,
    the layout of ``combineDescriptors``) for SVM fusion.  ``submit_video`` runs one video ahead of the read-back: video
    i + 1 is enqueued before the host waits for video i.

    On a pipeline with the RGB-difference stream (``rgb_diff=True``) the result is
    ``(acc_spatial, acc_temporal, acc_fused, descriptors, acc_difference)`` with descriptors ``[N,768]`` (spatial, temporal,
    difference) and ``fusion_weights`` of three entries.

    On a pipeline with ``heads`` ``task=`` travels through ``kw`` to ``submit_video``: the videos of one
    call belong to one dataset, the scores are that head's and ``labels`` are local to it.

    Decoded frames: an entry of ``videos`` may be ``(rgb, None)`` or ``rgb`` alone, and ``rescale=`` travels
    through ``kw``: ``submit_video`` then rescales the frames and derives the gray frames on the device.

    Stored flow: ``flows`` is an iterable parallel to ``videos``, one stored flow per video
    (``TwoStreamPipeline.extract_flow``), handed to ``submit_video(flow=)``: no TV-L1 runs, and the videos come without gray
    frames.  Fewer or more stored flows than videos raise ValueError.

    Motion-JPEG files: an entry of ``videos`` may be the path of a Motion-JPEG AVI; ``submit_video``
    decodes its frames on the device."""
    labels = [int(l) for l in labels]
    stored = iter(flows) if flows is not None else None
    missing = object()
    rows, pending, n = [], None, 0
    third = getattr(pipe, "diff", None) is not None
    keys = ("scores_s", "scores_t", "pred", "desc_s", "desc_t") + (("desc_d", "scores_d") if third else ())

    def collect(out):
        out["done"].synchronize()
        rows.append(tuple(out[key].cpu().numpy() for key in keys))

    for v in videos:
        rgb, gray = v if isinstance(v, (tuple, list)) else (v, None)
        if stored is not None:
            f = next(stored, missing)
            if f is missing:
                raise ValueError("evaluateVideos: fewer stored flows than videos")
            out = pipe.submit_video(rgb, gray, flow=f, **kw)
        else:
            out = pipe.submit_video(rgb, gray, **kw)
        n += 1
        if pending is not None:
            collect(pending)
        pending = out
    if pending is not None:
        collect(pending)
    pipe.wait()
    if stored is not None and next(stored, missing) is not missing:
        raise ValueError("evaluateVideos: more stored flows than videos")
    if n != len(labels):
        raise ValueError("evaluateVideos: %d videos but %d labels" % (n, len(labels)))
    if n == 0:
        raise ValueError("evaluateVideos: no videos")
    y = np.asarray(labels)
    acc_s = float(np.mean(np.array([int(np.argmax(r[0])) for r in rows]) == y))
    acc_t = float(np.mean(np.array([int(np.argmax(r[1])) for r in rows]) == y))
    acc_f = float(np.mean(np.array([int(r[2]) for r in rows]) == y))
    desc = np.stack([np.concatenate(r[3:6]) for r in rows]).astype(np.float32)
    if third:
        acc_d = float(np.mean(np.array([int(np.argmax(r[6])) for r in rows]) == y))
        return acc_s, acc_t, acc_f, desc, acc_d
    return acc_s, acc_t, acc_f, desc
