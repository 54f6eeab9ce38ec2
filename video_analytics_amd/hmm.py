"""HMM action segmentation on MI355X (``csrc/hmm.hip``): the modelled project's Sheet04 (Kuehne, Arslan
and Serre, CVPR 2014) -- one diagonal Gaussian per sub-action state, units composed into one flat model per grammar
(``GrammarContext``, Sheet04.py:197-274), Viterbi decoding of every (video, grammar) pair (Sheet04.py:520-560, 583-602) and
Baum-Welch training on isolated unit sequences (Sheet04.py:284-513).

The features are CUDA float32 or float64 rows (what ``fisher.pca_transform`` leaves: 64 columns, ``GMM_DIM`` of
Sheet04.py:10).  The emission table ``logB [frames, G]`` is computed once per video and shared by every grammar; a pair is one
workgroup's chain of adds and maxima in float64, so scores and paths are exact statements of S99, the same bits on every
call.  Thousands of pairs run in one launch; all pairs are scored without backpointers and only the winners are decoded.
Training runs the scaled forward-backward recursion (S100) over every sequence in one launch, sums the Gaussian statistics on
the device in a written order (S101) and takes the M-step on the host (S102: G x D numbers).

Where it departs from Sheet04.py, deliberately: the first frame adds the start log-probability to the
emission instead of multiplying them, the path ends in a state weighted by the last unit's exit and starts where ``log_pi``
allows, scores include the transitions, beta runs backwards under alpha's scales, a starved state keeps its parameters, and
the caller's matrices are never written to.
"""
import math

import numpy as np
import torch

from . import _ffi
from ._features import check_segments, dev64, workspace

MAX_DIM, MAX_STATES = _ffi.HMM_MAX_DIM, _ffi.HMM_MAX_STATES
MEMORY_BUDGET_BYTES = 1 << 30  # the backpointers and paths of one round of decoded jobs
STATUS_OK, STATUS_NO_PATH, STATUS_NAN = 0, 1, 2
NEG_INF = float("-inf")


def wave_states():
    """The states (and ``wave_edges()`` the edges) up to which a model runs in the kernel's single-wave form."""
    return int(_ffi.lib().va_hmm_wave_states())


def wave_edges():
    return int(_ffi.lib().va_hmm_wave_edges())


def backtrack_block():
    """The frames of backpointers that pass through LDS per step of the backtrack."""
    return int(_ffi.lib().va_hmm_backtrack_block())


def _log(p):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(p, dtype=np.float64))


def _no_nan(a, who, name):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if np.isnan(a).any() or (a == np.inf).any():
        raise ValueError("%s: %s must hold log-probabilities (finite or -inf), got a NaN or +inf" % (who, name))
    return a


class Unit(object):
    """One action unit: ``n`` states that own the Gaussians ``first .. first + n - 1`` of their ``HmmSet``, with ``log_pi
    [n]``, ``log_a [n,n]`` (row: from, column: to) and ``exit_logp [n]``, all float64 log-probabilities; -inf is legal."""

    def __init__(self, name, first, log_pi, log_a, exit_logp):
        who = "Unit"
        self.name, self.first = str(name), int(first)
        self.log_pi = _no_nan(log_pi, who, "log_pi")
        self.log_a = _no_nan(log_a, who, "log_a")
        self.exit_logp = _no_nan(exit_logp, who, "exit_logp")
        n = self.log_pi.shape[0] if self.log_pi.ndim == 1 else 0
        if n < 1 or self.log_a.shape != (n, n) or self.exit_logp.shape != (n,):
            raise ValueError("%s %r: need log_pi [n], log_a [n,n] and exit_logp [n] with n >= 1, got %s, %s and %s"
                             % (who, self.name, self.log_pi.shape, self.log_a.shape, self.exit_logp.shape))
        if self.first < 0:
            raise ValueError("%s %r: first must be >= 0, got %d" % (who, self.name, self.first))

    @property
    def n_states(self):
        return int(self.log_pi.shape[0])


class Model(object):
    """A flat model in CSR form by predecessor (include/va.h): ``emit int32 [N]``, ``pred_ptr int32 [N + 1]``, ``pred_idx int32
    [E]`` ascending within a state, ``pred_logp float64 [E]``, ``log_pi`` and ``log_final float64 [N]``.  ``unit_of_state int32
    [N]`` (optional) is the position in the composed sequence each state belongs to, and ``units`` that sequence's unit indices
    in the ``HmmSet``."""

    def __init__(self, emit, pred_ptr, pred_idx, pred_logp, log_pi, log_final, unit_of_state=None, units=None):
        who = "Model"
        self.emit = np.ascontiguousarray(emit, dtype=np.int32)
        self.pred_ptr = np.ascontiguousarray(pred_ptr, dtype=np.int32)
        self.pred_idx = np.ascontiguousarray(pred_idx, dtype=np.int32)
        self.pred_logp = _no_nan(pred_logp, who, "pred_logp")
        self.log_pi = _no_nan(log_pi, who, "log_pi")
        self.log_final = _no_nan(log_final, who, "log_final")
        n = int(self.emit.shape[0]) if self.emit.ndim == 1 else 0
        if not 1 <= n <= MAX_STATES:
            raise ValueError("%s: need 1 <= N <= %d states, got emit of shape %s" % (who, MAX_STATES, self.emit.shape))
        if self.pred_ptr.shape != (n + 1,) or self.log_pi.shape != (n,) or self.log_final.shape != (n,):
            raise ValueError("%s: pred_ptr must be [N + 1], log_pi and log_final [N] for N = %d" % (who, n))
        e = int(self.pred_ptr[-1])
        if self.pred_ptr[0] != 0 or (np.diff(self.pred_ptr) < 0).any() or self.pred_idx.shape != (e,) or self.pred_logp.shape != (e,):
            raise ValueError("%s: pred_ptr must ascend from 0 to E, the length of pred_idx and pred_logp" % who)
        if (self.emit < 0).any():
            raise ValueError("%s: emit must be >= 0" % who)
        if e and ((self.pred_idx < 0).any() or (self.pred_idx >= n).any()):
            raise ValueError("%s: pred_idx must lie in 0 .. N - 1" % who)
        if e > 1:
            inner = np.ones(e - 1, dtype=bool)  # True where two neighbouring edges belong to one state
            cuts = self.pred_ptr[1:-1]
            inner[cuts[(cuts > 0) & (cuts < e)] - 1] = False
            if (np.diff(self.pred_idx)[inner] <= 0).any():
                raise ValueError("%s: pred_idx must ascend strictly within a state" % who)
        self.unit_of_state = None if unit_of_state is None else np.ascontiguousarray(unit_of_state, dtype=np.int32)
        self.units = None if units is None else [int(u) for u in units]
        if self.unit_of_state is not None and self.unit_of_state.shape != (n,):
            raise ValueError("%s: unit_of_state must be [N]" % who)

    @property
    def n_states(self):
        return int(self.emit.shape[0])

    @property
    def n_edges(self):
        return int(self.pred_idx.shape[0])

    @classmethod
    def from_dense(cls, log_a, log_pi, log_final, emit=None):
        """The model of a dense ``log_a [N,N]`` (row: from, column: to): an edge for every entry above -inf."""
        log_a = _no_nan(log_a, "Model.from_dense", "log_a")
        n = log_a.shape[0]
        if log_a.ndim != 2 or log_a.shape != (n, n):
            raise ValueError("Model.from_dense: log_a must be [N,N], got %s" % (log_a.shape,))
        ptr, idx, lp = [0], [], []
        for j in range(n):
            i = np.nonzero(log_a[:, j] > NEG_INF)[0]
            idx.append(i)
            lp.append(log_a[i, j])
            ptr.append(ptr[-1] + len(i))
        return cls(np.arange(n) if emit is None else emit, ptr, np.concatenate(idx), np.concatenate(lp), log_pi, log_final)


class HmmSet(object):
    """``G`` diagonal Gaussians (float64 ``means [G,D]`` and ``variances [G,D]``, D <= 512) and a list of named units, each
    owning a contiguous run of them as its states (S97)."""

    def __init__(self, means, variances, units=()):
        who = "HmmSet"
        self.means = np.ascontiguousarray(means, dtype=np.float64)
        self.variances = np.ascontiguousarray(variances, dtype=np.float64)
        if self.means.ndim != 2 or self.means.shape != self.variances.shape or self.means.shape[0] < 1 or not 1 <= self.means.shape[1] <= MAX_DIM:
            raise ValueError("%s: means and variances must be [G, D] with G >= 1 and 1 <= D <= %d, got %s and %s"
                             % (who, MAX_DIM, self.means.shape, self.variances.shape))
        if not np.isfinite(self.means).all() or not np.isfinite(self.variances).all() or not (self.variances > 0).all():
            raise ValueError("%s: means must be finite and variances finite and > 0" % who)
        self.units = []
        for u in units:
            self.add_unit(u)

    @property
    def n_gaussians(self):
        return int(self.means.shape[0])

    @property
    def dim(self):
        return int(self.means.shape[1])

    @property
    def names(self):
        return [u.name for u in self.units]

    def add_unit(self, unit):
        if not isinstance(unit, Unit):
            raise ValueError("HmmSet.add_unit: not a Unit: %r" % (unit,))
        if unit.name in self.names:
            raise ValueError("HmmSet.add_unit: a unit named %r exists already" % unit.name)
        if unit.first + unit.n_states > self.n_gaussians:
            raise ValueError("HmmSet.add_unit: unit %r owns Gaussians %d .. %d, the set has %d"
                             % (unit.name, unit.first, unit.first + unit.n_states - 1, self.n_gaussians))
        self.units.append(unit)
        return unit

    @staticmethod
    def left_to_right(name, first, n_states, self_prob=0.9, next_prob=0.1):
        """The default topology, Sheet04's (Sheet04.py:13-14, 127-144): every state stays with ``self_prob`` and moves on with
        ``next_prob``; the last state's move is the unit's exit; the unit starts in its first state."""
        n = int(n_states)
        if n < 1:
            raise ValueError("HmmSet.left_to_right: n_states must be >= 1, got %d" % n)
        for label, p in (("self_prob", self_prob), ("next_prob", next_prob)):
            if not 0.0 <= float(p) <= 1.0:
                raise ValueError("HmmSet.left_to_right: %s must lie in [0, 1], got %r" % (label, p))
        a = np.zeros((n, n))
        for i in range(n):
            a[i, i] = self_prob
            if i + 1 < n:
                a[i, i + 1] = next_prob
        pi, ex = np.zeros(n), np.zeros(n)
        pi[0], ex[n - 1] = 1.0, next_prob
        return HmmSet.unit_from_dense(name, first, a, pi, ex)

    @staticmethod
    def unit_from_dense(name, first, A, pi, exit):
        """A unit of any topology from probabilities: ``A [n,n]`` (row: from), ``pi [n]`` and ``exit [n]``; zeros become -inf."""
        for label, v in (("A", A), ("pi", pi), ("exit", exit)):
            v = np.asarray(v, dtype=np.float64)
            if not np.isfinite(v).all() or (v < 0).any():
                raise ValueError("HmmSet.unit_from_dense: %s must hold finite probabilities >= 0" % label)
        return Unit(name, first, _log(pi), _log(A), _log(exit))

    def unit_index(self, name):
        try:
            return self.names.index(name)
        except ValueError:
            raise ValueError("HmmSet: no unit named %r" % (name,))

    def compose(self, unit_names):
        """The flat model of a sequence of units (S97): the units one after another, an edge from state s of unit k to state
        s' of unit k + 1 with ``exit[s] + log_pi[s']``, the first unit's ``log_pi`` as the start and the last unit's ``exit`` as
        the end weight.  Edges of -inf are left out: by S99's strict ``>`` they could never win."""
        if isinstance(unit_names, str) or len(unit_names) == 0:
            raise ValueError("HmmSet.compose: unit_names must be a non-empty list of unit names")
        seq = [self.unit_index(nm) for nm in unit_names]
        units = [self.units[i] for i in seq]
        n = sum(u.n_states for u in units)
        if n > MAX_STATES:
            raise ValueError("HmmSet.compose: the sequence has %d states, a model holds at most %d" % (n, MAX_STATES))
        emit, unit_of_state, ptr, idx, lp = [], [], [0], [], []
        log_pi, log_final = np.full(n, NEG_INF), np.full(n, NEG_INF)
        base = 0
        for k, u in enumerate(units):
            prev = units[k - 1] if k > 0 else None
            for s2 in range(u.n_states):
                if prev is not None:
                    for s in range(prev.n_states):
                        w = prev.exit_logp[s] + u.log_pi[s2] if prev.exit_logp[s] > NEG_INF and u.log_pi[s2] > NEG_INF else NEG_INF
                        if w > NEG_INF:
                            idx.append(base - prev.n_states + s)
                            lp.append(w)
                for s in range(u.n_states):
                    if u.log_a[s, s2] > NEG_INF:
                        idx.append(base + s)
                        lp.append(u.log_a[s, s2])
                ptr.append(len(idx))
                emit.append(u.first + s2)
                unit_of_state.append(k)
            if k == 0:
                log_pi[:u.n_states] = u.log_pi
            if k == len(units) - 1:
                log_final[base:] = u.exit_logp
            base += u.n_states
        return Model(emit, ptr, idx, lp, log_pi, log_final, unit_of_state, seq)

    def save(self, path):
        save_hmmset(self, path)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return load_hmmset(z)

    def emission_constants(self):
        """What ``va_hmm_emissions`` takes from the host, in float64: ``iv = 1 / var [G,D]`` and ``c [G] = -0.5 (D log 2 pi +
        sum_d log var)``, the logarithms added over the columns in ascending order."""
        iv = 1.0 / self.variances
        s = np.zeros(self.n_gaussians)
        for c in range(self.dim):
            s = s + np.log(self.variances[:, c])
        return iv, -0.5 * (self.dim * math.log(2.0 * math.pi) + s)


def _rows(x, who, name="x", max_dim=MAX_DIM):
    """A CUDA float32 or float64 ``[n, d]`` tensor with 1 .. ``max_dim`` columns (None: any number, an emission table's), or a
    list of them -> (one contiguous tensor, segments or None).  ``_features.check_rows`` and ``check_videos`` say the same for
    float32 alone; S98 takes float64 rows too."""
    if isinstance(x, (list, tuple)):
        if len(x) == 0:
            raise ValueError("%s: %s is an empty list" % (who, name))
        parts = [_rows(p, who, name, max_dim)[0] for p in x]
        if len(set((int(p.shape[1]), p.dtype, p.device) for p in parts)) != 1:
            raise ValueError("%s: the tensors of %s must share one width, one dtype and one device" % (who, name))
        seg = np.concatenate([[0], np.cumsum([int(p.shape[0]) for p in parts])]).astype(np.int64)
        return (torch.cat(parts, 0) if len(parts) > 1 else parts[0]), seg
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("%s: %s must be a CUDA tensor or a list of CUDA tensors" % (who, name))
    if x.dim() != 2 or x.dtype not in (torch.float32, torch.float64):
        raise ValueError("%s: %s must be float32 or float64 [n, d], got %s %s" % (who, name, x.dtype, tuple(x.shape)))
    if x.shape[1] < 1 or (max_dim is not None and x.shape[1] > max_dim):
        raise ValueError("%s: %s must have 1 .. %s columns, got %d" % (who, name, "any number of" if max_dim is None else max_dim, x.shape[1]))
    return x.contiguous(), None


def emissions(x, hmmset):
    """``va_hmm_emissions`` (S98): x CUDA float32 or float64 ``[T, D]`` (or a list of such tensors, concatenated) -> CUDA
    float64 ``logB [T, G]``, ``logB[t,g] = c_g - 0.5 sum_d ((x_d - mu_gd)(x_d - mu_gd)) / var_gd`` with the columns in ascending
    order: the bits of the numpy loop that states it."""
    who = "emissions"
    if not isinstance(hmmset, HmmSet):
        raise ValueError("%s: hmmset must be an HmmSet" % who)
    x, _ = _rows(x, who)
    t, d, dev = int(x.shape[0]), int(x.shape[1]), x.device
    if d != hmmset.dim:
        raise ValueError("%s: x has %d columns, the Gaussians %d" % (who, d, hmmset.dim))
    g = hmmset.n_gaussians
    if t == 0:
        return torch.empty((0, g), dtype=torch.float64, device=dev)
    iv, c = hmmset.emission_constants()
    mu_d, iv_d, c_d = dev64(hmmset.means, dev), dev64(iv, dev), dev64(c, dev)
    logb = torch.empty((t, g), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _ffi.check(_ffi.lib().va_hmm_emissions(_ffi.ctx(dev.index), _ffi.ptr(x), int(x.dtype == torch.float64), t, d, _ffi.ptr(mu_d),
                                               _ffi.ptr(iv_d), _ffi.ptr(c_d), g, _ffi.ptr(logb), _ffi.stream_ptr(dev)))
    return logb


def check_jobs(jobs, n_seqs, n_models, who="viterbi"):
    """``jobs``: None (every (sequence, model) pair, decoded) or integers ``[J, 3]`` of (sequence, model, want_path) -> int32."""
    if jobs is None:
        return np.array([(s, m, 1) for s in range(n_seqs) for m in range(n_models)], dtype=np.int32).reshape(-1, 3)
    j = np.asarray(jobs.cpu() if isinstance(jobs, torch.Tensor) else jobs)
    if j.ndim != 2 or j.shape[1] != 3 or j.shape[0] < 1 or j.dtype.kind not in "iu":
        raise ValueError("%s: jobs must be integers [J, 3] of (sequence, model, want_path) with J >= 1" % who)
    j = j.astype(np.int64)
    if (j[:, 0] < 0).any() or (j[:, 0] >= n_seqs).any():
        raise ValueError("%s: jobs name a sequence outside 0 .. %d" % (who, n_seqs - 1))
    if (j[:, 1] < 0).any() or (j[:, 1] >= n_models).any():
        raise ValueError("%s: jobs name a model outside 0 .. %d" % (who, n_models - 1))
    if ((j[:, 2] != 0) & (j[:, 2] != 1)).any():
        raise ValueError("%s: want_path must be 0 or 1" % who)
    return np.ascontiguousarray(j.astype(np.int32))


def plan_rounds(need_bytes, want, budget, who, lengths, states):
    """Cuts the jobs, in their order, into rounds whose wanted jobs' ``need_bytes`` fit ``budget``: -> a list of (first job,
    one past the last).  A job that alone does not fit raises ValueError by name."""
    rounds, first, used = [], 0, 0
    for i, (b, w) in enumerate(zip(need_bytes, want)):
        need = int(b) if w else 0
        if need > budget:
            raise ValueError("%s: job %d alone (%d frames x %d states) needs %d bytes, more than memory_budget (%d)"
                             % (who, i, lengths[i], states[i], need, budget))
        if used + need > budget:
            rounds.append((first, i))
            first, used = i, 0
        used += need
    rounds.append((first, len(need_bytes)))
    return rounds


class _Packed(object):
    """The models of a call, concatenated on the device as include/va.h lays them out."""

    def __init__(self, models, g, dev, who):
        if isinstance(models, Model):
            models = [models]
        if not isinstance(models, (list, tuple)) or len(models) == 0 or not all(isinstance(m, Model) for m in models):
            raise ValueError("%s: models must be a non-empty list of Model" % who)
        for i, m in enumerate(models):
            if int(m.emit.max()) >= g:
                raise ValueError("%s: model %d emits Gaussian %d, logB has %d columns" % (who, i, int(m.emit.max()), g))
        self.n_states = np.array([m.n_states for m in models], dtype=np.int64)
        self.state_ptr = np.concatenate([[0], np.cumsum(self.n_states)]).astype(np.int32)
        self.edge_ptr = np.concatenate([[0], np.cumsum([m.n_edges for m in models])]).astype(np.int32)

        def cat(name, dtype):
            return torch.as_tensor(np.ascontiguousarray(np.concatenate([getattr(m, name) for m in models]).astype(dtype))).to(dev)
        self.emit, self.pred_ptr, self.pred_idx = cat("emit", np.int32), cat("pred_ptr", np.int32), cat("pred_idx", np.int32)
        self.pred_logp, self.log_pi, self.log_final = cat("pred_logp", np.float64), cat("log_pi", np.float64), cat("log_final", np.float64)
        self.state_ptr_d, self.edge_ptr_d = torch.as_tensor(self.state_ptr).to(dev), torch.as_tensor(self.edge_ptr).to(dev)
        self.n_models, self.models, self.dev = len(models), list(models), dev
        self.n_edges = np.array([m.n_edges for m in models], dtype=np.int64)

    def successors(self):
        """The successor lists of ``va_hmm_forward_backward``, on the device: (succ_ptr, succ_idx, succ_edge)."""
        rows = [successor_lists(m) for m in self.models]
        return tuple(torch.as_tensor(np.ascontiguousarray(np.concatenate([r[i] for r in rows]).astype(np.int32))).to(self.dev)
                     for i in range(3))

    def args(self):
        """The arguments every batched entry point takes after ``seq_ptr`` and ``n_seqs``."""
        return (_ffi.ptr(self.state_ptr_d), _ffi.ptr(self.edge_ptr_d), self.n_models, int(self.state_ptr[-1]), int(self.edge_ptr[-1]),
                _ffi.ptr(self.emit), _ffi.ptr(self.pred_ptr), _ffi.ptr(self.pred_idx), _ffi.ptr(self.pred_logp), _ffi.ptr(self.log_pi),
                _ffi.ptr(self.log_final))


def successor_lists(model):
    """The edges of a ``Model`` by source: -> ``(succ_ptr int32 [N + 1], succ_idx int32 [E], succ_edge int32 [E])``, the targets
    of every state in ascending order and each edge's place in ``pred_idx``."""
    n = model.n_states
    tgt = np.repeat(np.arange(n), np.diff(model.pred_ptr))
    src = model.pred_idx
    order = np.lexsort((tgt, src))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))])
    return ptr.astype(np.int32), tgt[order].astype(np.int32), order.astype(np.int32)


def _batch(who, logb_or_x, models, jobs, segments, hmmset, memory_budget):
    """The front end of ``viterbi`` and ``forward_backward``: -> (table, segments, packed models, jobs, budget)."""
    table, seg = _rows(logb_or_x, who, "logb_or_x", MAX_DIM if hmmset is not None else None)
    if seg is not None and segments is not None:
        raise ValueError("%s: segments comes with one tensor; a list carries its own" % who)
    if hmmset is not None:
        table = emissions(table, hmmset)
    if table.dtype != torch.float64:
        raise ValueError("%s: the emission table must be float64 (pass hmmset to compute it from features)" % who)
    t_total, g, dev = int(table.shape[0]), int(table.shape[1]), table.device
    if seg is None:
        seg = np.array([0, t_total], dtype=np.int64) if segments is None else check_segments(segments, t_total, who)
    if t_total < 1 or (np.diff(seg) < 1).any():
        raise ValueError("%s: every sequence must hold at least one frame" % who)
    budget = MEMORY_BUDGET_BYTES if memory_budget is None else int(memory_budget)
    pk = _Packed(models, g, dev, who)
    return table, seg, pk, check_jobs(jobs, len(seg) - 1, pk.n_models, who), budget


def viterbi(logb_or_x, models, jobs=None, segments=None, hmmset=None, memory_budget=None):
    """``va_hmm_viterbi`` (S99) over a batch of (sequence, model) jobs.

    ``logb_or_x``: the emission table, CUDA float64 ``[T_total, G]`` with ``segments [S + 1]`` (ascending frame offsets from 0;
    None: one sequence), or a list of per-sequence tables; with ``hmmset`` given it is the features instead and the table is
    computed here.  ``models``: a list of ``Model``.  ``jobs``: integers ``[J, 3]`` of (sequence, model, want_path), or None for
    every pair, decoded.  Every sequence holds at least one frame.

    -> ``(scores float64 [J], status int32 [J], paths)``, numpy; ``paths[i]`` is the int32 state per frame of a job that wanted
    it (all -1 unless its status is 0) and None otherwise.  Status 1: no path of finite score (score -inf); 2: a NaN reached
    the recursion (score NaN).  The jobs run in rounds whose backpointers fit ``memory_budget`` (default
    ``MEMORY_BUDGET_BYTES``); a job that alone does not fit raises ValueError."""
    who = "viterbi"
    table, seg, pk, jobs, budget = _batch(who, logb_or_x, models, jobs, segments, hmmset, memory_budget)
    t_total, g, dev, n_seqs = int(table.shape[0]), int(table.shape[1]), table.device, len(seg) - 1
    lengths = np.diff(seg)[jobs[:, 0]]
    states = pk.n_states[jobs[:, 1]]
    rounds = plan_rounds(2 * lengths * states + 4 * lengths, jobs[:, 2], budget, who, lengths, states)
    seg_d = torch.as_tensor(seg.astype(np.int32)).to(dev)
    n_jobs = len(jobs)
    scores, status, paths = np.empty(n_jobs, dtype=np.float64), np.empty(n_jobs, dtype=np.int32), [None] * n_jobs
    L = _ffi.lib()
    for lo, hi in rounds:
        jr, want = jobs[lo:hi], jobs[lo:hi, 2].astype(bool)
        path_len = np.where(want, lengths[lo:hi], 0).astype(np.int64)
        bp_len = path_len * states[lo:hi]
        path_off = np.concatenate([[0], np.cumsum(path_len)]).astype(np.int64)
        bp_off = np.concatenate([[0], np.cumsum(bp_len)]).astype(np.int64)
        path_elems, bp_elems = int(path_off[-1]), int(bp_off[-1])
        jobs_d = torch.as_tensor(np.ascontiguousarray(jr)).to(dev)
        po_d, bo_d = torch.as_tensor(path_off[:-1].copy()).to(dev), torch.as_tensor(bp_off[:-1].copy()).to(dev)
        score_d = torch.empty((hi - lo,), dtype=torch.float64, device=dev)
        status_d = torch.empty((hi - lo,), dtype=torch.int32, device=dev)
        path_d = torch.empty((max(path_elems, 1),), dtype=torch.int32, device=dev)
        ws = workspace(2 * bp_elems, dev) if bp_elems else None
        with torch.cuda.device(dev):
            _ffi.check(L.va_hmm_viterbi(
                _ffi.ctx(dev.index), _ffi.ptr(table), t_total, g, _ffi.ptr(seg_d), n_seqs, *pk.args(), _ffi.ptr(jobs_d), hi - lo,
                _ffi.ptr(po_d), _ffi.ptr(bo_d), _ffi.ptr(score_d), _ffi.ptr(status_d), _ffi.ptr(path_d), path_elems, bp_elems,
                _ffi.ptr(ws), 2 * bp_elems, _ffi.stream_ptr(dev)))
        scores[lo:hi], status[lo:hi] = score_d.cpu().numpy(), status_d.cpu().numpy()
        if (status[lo:hi] > STATUS_NAN).any():
            raise RuntimeError("%s: the library refused job %d as outside the call's arrays" % (who, lo + int(np.argmax(status[lo:hi] > STATUS_NAN))))
        if path_elems:
            flat = path_d.cpu().numpy()
            for i in np.nonzero(want)[0]:
                paths[lo + i] = flat[path_off[i]:path_off[i + 1]].copy()
    return scores, status, paths


def best_grammar(scores):
    """The arg-max over the grammars of ``scores [videos, grammars]``, the first on ties; a NaN counts as -inf."""
    s = np.where(np.isnan(scores), NEG_INF, np.asarray(scores, dtype=np.float64))
    return np.argmax(s, axis=1).astype(np.int64)


def boundaries(units):
    """The runs of a per-frame label sequence: -> a list of ``(first frame, one past the last, label)``."""
    units = np.asarray(units)
    if len(units) == 0:
        return []
    cut = np.concatenate([[0], np.nonzero(units[1:] != units[:-1])[0] + 1, [len(units)]])
    return [(int(a), int(b), int(units[a])) for a, b in zip(cut[:-1], cut[1:])]


class Decoded(object):
    """One decoded (video, grammar) pair: ``path`` (the model's state per frame), ``units`` (the ``HmmSet``'s unit index per
    frame), ``segments`` (``boundaries(units)`` with a repeated unit of the grammar kept apart) and the job's ``status``."""

    def __init__(self, path, model, status):
        self.path, self.status = path, int(status)
        if self.status == STATUS_OK:
            pos = model.unit_of_state[path]
            self.units = np.asarray(model.units, dtype=np.int32)[pos]
            self.segments = [(a, b, model.units[p]) for a, b, p in boundaries(pos)]
        else:
            self.units, self.segments = np.full(len(path), -1, dtype=np.int32), []


class Segmentation(object):
    """What ``segment`` returns: float64 ``scores [videos, grammars]``, int32 ``status`` of the same shape, ``best [videos]``
    and ``decoded``: ``{(video, grammar): Decoded}`` for the decoded pairs."""

    def __init__(self, scores, status, best, decoded):
        self.scores, self.status, self.best, self.decoded = scores, status, best, decoded

    def units(self, video):
        """The unit per frame of ``video`` under its best grammar."""
        return self.decoded[(int(video), int(self.best[video]))].units


def segment(features, hmmset, grammars, decode="best", segments=None, memory_budget=None):
    """Recognition and segmentation as Sheet04.py:583-602 runs it: every video against every grammar.

    ``features``: CUDA float32 or float64 ``[frames, D]`` with ``segments [videos + 1]``, or a list of per-video tensors.
    ``grammars``: a list of unit-name sequences.  The emission table is computed once and shared by the grammars; all pairs
    are scored without backpointers; then ``decode="best"`` decodes each video under its best grammar, ``"all"`` every pair and
    ``"none"`` nothing.  -> ``Segmentation``."""
    who = "segment"
    if decode not in ("best", "all", "none"):
        raise ValueError("%s: decode must be 'best', 'all' or 'none', got %r" % (who, decode))
    if not isinstance(hmmset, HmmSet):
        raise ValueError("%s: hmmset must be an HmmSet" % who)
    if isinstance(grammars, str) or len(grammars) == 0:
        raise ValueError("%s: grammars must be a non-empty list of unit-name sequences" % who)
    x, seg = _rows(features, who, "features")
    if seg is not None and segments is not None:
        raise ValueError("%s: segments comes with one tensor; a list carries its own" % who)
    if seg is None:
        seg = np.array([0, int(x.shape[0])], dtype=np.int64) if segments is None else check_segments(segments, int(x.shape[0]), who)
    models = [hmmset.compose(g) for g in grammars]
    logb = emissions(x, hmmset)
    nv, ng = len(seg) - 1, len(models)
    pairs = np.array([(v, g, 0) for v in range(nv) for g in range(ng)], dtype=np.int32)
    scores, status, _ = viterbi(logb, models, pairs, segments=seg, memory_budget=memory_budget)
    scores, status = scores.reshape(nv, ng), status.reshape(nv, ng)
    best = best_grammar(scores)
    decoded = {}
    if decode != "none":
        todo = [(v, int(best[v]), 1) for v in range(nv)] if decode == "best" else [(v, g, 1) for v in range(nv) for g in range(ng)]
        _, st, paths = viterbi(logb, models, np.array(todo, dtype=np.int32), segments=seg, memory_budget=memory_budget)
        for (v, g, _w), s, p in zip(todo, st, paths):
            decoded[(v, g)] = Decoded(p, models[g], s)
    return Segmentation(scores, status, best, decoded)


def mean_over_frames(pred_units, true_units):
    """The share of frames whose predicted unit equals the true one (Sheet04.py:165-177, with equality in place of its
    ``startswith``).  Each argument is one label sequence or a list of them; the frames of all sequences count alike."""
    def flat(u):
        if isinstance(u, (list, tuple)) and len(u) and not np.isscalar(u[0]):
            return np.concatenate([np.asarray(a).ravel() for a in u])
        return np.asarray(u).ravel()
    p, t = flat(pred_units), flat(true_units)
    if p.shape != t.shape or p.size == 0:
        raise ValueError("mean_over_frames: the sequences must have equal, non-zero lengths, got %d and %d" % (p.size, t.size))
    return float(np.count_nonzero(p == t)) / p.size


# ---- S100 forward-backward and the statistics -------------------------------------------------------------------------------

def _fb_rounds(who, table, seg, pk, jobs, budget):
    """``va_hmm_forward_backward`` round by round: yields ``(lo, hi, gamma (CUDA float64, the round's jobs one after another),
    gamma_off int64 [hi - lo + 1], xi_off likewise, xi numpy, loglik numpy, status numpy)``."""
    t_total, g, dev, n_seqs = int(table.shape[0]), int(table.shape[1]), table.device, len(seg) - 1
    lengths, states, edges = np.diff(seg)[jobs[:, 0]].astype(np.int64), pk.n_states[jobs[:, 1]], pk.n_edges[jobs[:, 1]]
    rounds = plan_rounds(8 * lengths * states + 16 * lengths + 8 * edges, np.ones(len(jobs), dtype=bool), budget, who, lengths, states)
    seg_d = torch.as_tensor(seg.astype(np.int32)).to(dev)
    succ = pk.successors()
    L = _ffi.lib()
    for lo, hi in rounds:
        gamma_off = np.concatenate([[0], np.cumsum(lengths[lo:hi] * states[lo:hi])]).astype(np.int64)
        xi_off = np.concatenate([[0], np.cumsum(edges[lo:hi])]).astype(np.int64)
        mc_off = np.concatenate([[0], np.cumsum(2 * lengths[lo:hi])]).astype(np.int64)
        gamma_elems, xi_elems, mc_elems = int(gamma_off[-1]), int(xi_off[-1]), int(mc_off[-1])
        jobs_d = torch.as_tensor(np.ascontiguousarray(jobs[lo:hi])).to(dev)
        go_d, xo_d, mo_d = (torch.as_tensor(o[:-1].copy()).to(dev) for o in (gamma_off, xi_off, mc_off))
        gamma = torch.empty((gamma_elems,), dtype=torch.float64, device=dev)
        xi = torch.empty((max(xi_elems, 1),), dtype=torch.float64, device=dev)
        loglik = torch.empty((hi - lo,), dtype=torch.float64, device=dev)
        status = torch.empty((hi - lo,), dtype=torch.int32, device=dev)
        ws = workspace(L.va_hmm_fb_workspace_bytes(int(pk.state_ptr[-1]), int(pk.edge_ptr[-1]), mc_elems), dev)
        with torch.cuda.device(dev):
            _ffi.check(L.va_hmm_forward_backward(
                _ffi.ctx(dev.index), _ffi.ptr(table), t_total, g, _ffi.ptr(seg_d), n_seqs, *pk.args(), _ffi.ptr(succ[0]), _ffi.ptr(succ[1]),
                _ffi.ptr(succ[2]), _ffi.ptr(jobs_d), hi - lo, _ffi.ptr(go_d), _ffi.ptr(xo_d), _ffi.ptr(mo_d), _ffi.ptr(gamma), gamma_elems,
                _ffi.ptr(xi), xi_elems, mc_elems, _ffi.ptr(loglik), _ffi.ptr(status), _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr(dev)))
        st = status.cpu().numpy()
        if (st > STATUS_NAN).any():
            raise RuntimeError("%s: the library refused job %d as outside the call's arrays" % (who, lo + int(np.argmax(st > STATUS_NAN))))
        yield lo, hi, gamma, gamma_off, xi_off, xi.cpu().numpy()[:xi_elems], loglik.cpu().numpy(), st


def forward_backward(logb_or_x, models, jobs=None, segments=None, hmmset=None, memory_budget=None):
    """``va_hmm_forward_backward`` (S100) over a batch of (sequence, model) jobs; the arguments are ``viterbi``'s (the jobs'
    third column is not read).  -> ``(loglik float64 [J], status int32 [J], gamma, xi)``, numpy: ``gamma[k]`` the state
    posteriors ``[T, N]`` of job k and ``xi[k]`` its summed edge posteriors ``[E]``, in the order of the model's ``pred_idx``.
    Status 1: the likelihood is zero (``loglik`` -inf, zeros); 2: a NaN or +inf among the job's emissions (``loglik`` NaN,
    zeros)."""
    who = "forward_backward"
    table, seg, pk, jobs, budget = _batch(who, logb_or_x, models, jobs, segments, hmmset, memory_budget)
    n_jobs = len(jobs)
    loglik, status, gammas, xis = np.empty(n_jobs), np.empty(n_jobs, dtype=np.int32), [None] * n_jobs, [None] * n_jobs
    lengths, states = np.diff(seg)[jobs[:, 0]], pk.n_states[jobs[:, 1]]
    for lo, hi, gamma, gamma_off, xi_off, xi, ll, st in _fb_rounds(who, table, seg, pk, jobs, budget):
        loglik[lo:hi], status[lo:hi] = ll, st
        flat = gamma.cpu().numpy()
        for k in range(lo, hi):
            gammas[k] = flat[gamma_off[k - lo]:gamma_off[k - lo + 1]].reshape(int(lengths[k]), int(states[k])).copy()
            xis[k] = xi[xi_off[k - lo]:xi_off[k - lo + 1]].copy()
    return loglik, status, gammas, xis


def contributions(models, seg, jobs, gamma_off, n_gaussians):
    """The weights of ``va_hmm_gauss_stats``' gamma mode: for every Gaussian the (job, state) pairs that emit it, jobs ascending
    and states ascending within a job.  -> ``(contrib_ptr int32 [G + 1], contrib int32 [C, 4], contrib_off int64 [C])``."""
    gs, rows, offs = [], [], []
    for k, (s, m, _w) in enumerate(jobs):
        mod = models[m]
        n = mod.n_states
        gs.append(mod.emit.astype(np.int64))
        r = np.empty((n, 4), dtype=np.int64)
        r[:, 0], r[:, 1], r[:, 2], r[:, 3] = seg[s], seg[s + 1] - seg[s], n, np.arange(n)
        rows.append(r)
        offs.append(np.full(n, gamma_off[k], dtype=np.int64))
    gs, rows, offs = np.concatenate(gs), np.concatenate(rows), np.concatenate(offs)
    order = np.argsort(gs, kind="stable")  # the pairs are listed by job and state already
    ptr = np.concatenate([[0], np.cumsum(np.bincount(gs, minlength=n_gaussians))])
    return ptr.astype(np.int32), np.ascontiguousarray(rows[order].astype(np.int32)), np.ascontiguousarray(offs[order])


def _stats_call(x, n_gaussians, mode, gamma, contrib, align):
    t, d, dev = int(x.shape[0]), int(x.shape[1]), x.device
    stats = torch.empty((n_gaussians, 1 + 2 * d), dtype=torch.float64, device=dev)
    if mode == 0:
        cp, cr, co = (torch.as_tensor(a).to(dev) for a in contrib)
        args = (_ffi.ptr(gamma), int(gamma.numel()), _ffi.ptr(cp), _ffi.ptr(cr), _ffi.ptr(co), int(cr.shape[0]), _ffi.ptr(None))
    else:
        args = (_ffi.ptr(None), 0, _ffi.ptr(None), _ffi.ptr(None), _ffi.ptr(None), 0, _ffi.ptr(align))
    with torch.cuda.device(dev):
        _ffi.check(_ffi.lib().va_hmm_gauss_stats(_ffi.ctx(dev.index), _ffi.ptr(x), int(x.dtype == torch.float64), t, d, n_gaussians, mode,
                                                 *args, _ffi.ptr(stats), _ffi.stream_ptr(dev)))
    return stats


def gauss_stats(x, n_gaussians, align=None, gamma=None, models=None, jobs=None, segments=None):
    """``va_hmm_gauss_stats``: per Gaussian ``[sum w | sum w x | sum w x^2]`` as CUDA float64 ``[G, 1 + 2 D]``.  x: CUDA float32
    or float64 ``[T_total, D]`` (or a list).  Either ``align``: an int32 Gaussian per frame (-1: none), the hard alignment; or
    ``gamma``: the per-job posteriors ``forward_backward`` returned, with its ``models``, ``jobs`` and ``segments``."""
    who = "gauss_stats"
    x, seg = _rows(x, who)
    t, d, dev, g = int(x.shape[0]), int(x.shape[1]), x.device, int(n_gaussians)
    if t < 1 or g < 1:
        raise ValueError("%s: need at least one row and n_gaussians >= 1" % who)
    if (align is None) == (gamma is None):
        raise ValueError("%s: pass either align or gamma" % who)
    if align is not None:
        a = torch.as_tensor(np.ascontiguousarray(align.cpu().numpy() if isinstance(align, torch.Tensor) else align))
        if a.dim() != 1 or a.shape[0] != t or a.dtype not in (torch.int32, torch.int64):
            raise ValueError("%s: align must hold one integer per row of x (%d), got %s %s" % (who, t, a.dtype, tuple(a.shape)))
        return _stats_call(x, g, 1, None, None, a.to(torch.int32).to(dev).contiguous())
    if seg is None:
        seg = np.array([0, t], dtype=np.int64) if segments is None else check_segments(segments, t, who)
    if isinstance(models, Model):
        models = [models]
    if not models or not all(isinstance(m, Model) for m in models):
        raise ValueError("%s: the gamma mode needs the models of the jobs" % who)
    jobs = check_jobs(jobs, len(seg) - 1, len(models), who)
    if len(gamma) != len(jobs):
        raise ValueError("%s: %d jobs but %d gamma arrays" % (who, len(jobs), len(gamma)))
    for k, (s, m, _w) in enumerate(jobs):
        if np.shape(gamma[k]) != (seg[s + 1] - seg[s], models[m].n_states) or int(models[m].emit.max()) >= g:
            raise ValueError("%s: gamma[%d] must be [%d, %d] and its model emit below n_gaussians"
                             % (who, k, seg[s + 1] - seg[s], models[m].n_states))
    off = np.concatenate([[0], np.cumsum([np.size(a) for a in gamma])]).astype(np.int64)
    flat = dev64(np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in gamma]), dev)
    return _stats_call(x, g, 0, flat, contributions(models, seg, jobs, off, g), None)


# ---- the M-step (host, float64: G x D numbers) and fit ------------------------------------------------------------------------

def mstep_gaussians(stats, means, variances, var_floor, min_occupancy):
    """``mu = S1 / S0``, ``var = S2 / S0 - mu mu + var_floor``; a Gaussian whose ``S0`` is below ``min_occupancy`` (or not
    finite) keeps its parameters.  -> (means, variances)."""
    stats = np.asarray(stats, dtype=np.float64)
    d = means.shape[1]
    s0 = stats[:, 0]
    fed = np.isfinite(s0) & (s0 >= min_occupancy) & (s0 > 0)
    safe = np.where(fed, s0, 1.0)[:, None]
    mu = stats[:, 1:1 + d] / safe
    var = stats[:, 1 + d:] / safe - mu * mu + var_floor
    return np.where(fed[:, None], mu, means), np.where(fed[:, None], var, variances)


def mstep_unit(unit, xi_sum, start_sum, exit_sum):
    """A unit's transitions from the summed statistics: every row is renormalised over its out-edges (the unit's own edges,
    ``xi_sum [n, n]``) and its exit (``exit_sum [n]``), added in ascending order of the target with the exit last; a row
    without statistics is kept.  ``log_pi`` likewise from ``start_sum``.  An edge the unit lacks stays absent.  -> Unit."""
    n = unit.n_states
    log_a, exit_logp, log_pi = unit.log_a.copy(), unit.exit_logp.copy(), unit.log_pi.copy()
    for i in range(n):
        total = 0.0
        for j in range(n):
            if unit.log_a[i, j] > NEG_INF:
                total = total + xi_sum[i, j]
        if unit.exit_logp[i] > NEG_INF:
            total = total + exit_sum[i]
        if not (total > 0.0 and np.isfinite(total)):
            continue
        for j in range(n):
            if unit.log_a[i, j] > NEG_INF:
                log_a[i, j] = _log(xi_sum[i, j] / total)
        if unit.exit_logp[i] > NEG_INF:
            exit_logp[i] = _log(exit_sum[i] / total)
    total = 0.0
    for i in range(n):
        if unit.log_pi[i] > NEG_INF:
            total = total + start_sum[i]
    if total > 0.0 and np.isfinite(total):
        for i in range(n):
            if unit.log_pi[i] > NEG_INF:
                log_pi[i] = _log(start_sum[i] / total)
    return Unit(unit.name, unit.first, log_pi, log_a, exit_logp)


def uniform_alignment(t, n):
    """The uniform left-to-right split of ``t`` frames over ``n`` states: frame i belongs to state ``i n // t``."""
    return (np.arange(int(t), dtype=np.int64) * int(n)) // max(int(t), 1)


def _dense_xi(model, xi):
    """One job's edge sums, in the order of its single-unit model's ``pred_idx``, as the unit's ``[n, n]`` array."""
    n = model.n_states
    dense = np.zeros((n, n))
    dense[model.pred_idx, np.repeat(np.arange(n), np.diff(model.pred_ptr))] = xi
    return dense


def check_fit_args(n_seqs, unit_of_sequence, n_states, init_alignments, lengths, iters, method, var_floor, min_occupancy, self_prob,
                   next_prob):
    """The argument checks of ``fit`` that need no device: ValueError naming the argument.  -> (unit names in the order they
    first appear, states per unit)."""
    who = "fit"
    if len(unit_of_sequence) != n_seqs:
        raise ValueError("%s: %d sequences but %d entries of unit_of_sequence" % (who, n_seqs, len(unit_of_sequence)))
    names = []
    for nm in unit_of_sequence:
        if not isinstance(nm, str):
            raise ValueError("%s: unit_of_sequence must hold unit names, got %r" % (who, nm))
        if nm not in names:
            names.append(nm)
    if isinstance(n_states, dict):
        missing = [nm for nm in names if nm not in n_states]
        if missing:
            raise ValueError("%s: n_states lacks the units %s" % (who, missing))
        counts = [n_states[nm] for nm in names]
    else:
        counts = [n_states] * len(names)
    for c in counts:
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 1 <= c <= MAX_STATES:
            raise ValueError("%s: n_states must be integers in 1 .. %d, got %r" % (who, MAX_STATES, c))
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 0:
        raise ValueError("%s: iters must be an integer >= 0, got %r" % (who, iters))
    if method not in ("baum-welch", "viterbi"):
        raise ValueError("%s: method must be 'baum-welch' or 'viterbi', got %r" % (who, method))
    for label, v, lo in (("var_floor", var_floor, 0.0), ("min_occupancy", min_occupancy, 0.0)):
        if not isinstance(v, (int, float, np.integer, np.floating)) or isinstance(v, bool) or not np.isfinite(v) or v < lo:
            raise ValueError("%s: %s must be a finite number >= %g, got %r" % (who, label, lo, v))
    for label, v in (("self_prob", self_prob), ("next_prob", next_prob)):
        if not isinstance(v, (int, float, np.integer, np.floating)) or isinstance(v, bool) or not 0.0 < v <= 1.0:
            raise ValueError("%s: %s must lie in (0, 1], got %r" % (who, label, v))
    if init_alignments is not None:
        if len(init_alignments) != n_seqs:
            raise ValueError("%s: %d sequences but %d init_alignments" % (who, n_seqs, len(init_alignments)))
        for i, a in enumerate(init_alignments):
            a = np.asarray(a)
            n = counts[names.index(unit_of_sequence[i])]
            if a.shape != (lengths[i],) or a.dtype.kind not in "iu" or (a < 0).any() or (a >= n).any():
                raise ValueError("%s: init_alignments[%d] must hold one state in 0 .. %d per frame (%d frames)" % (who, i, n - 1, lengths[i]))
    return names, [int(c) for c in counts]


def fit(sequences, unit_of_sequence, n_states, init_alignments=None, iters=5, method="baum-welch", var_floor=1e-6, min_occupancy=1e-3,
        self_prob=0.9, next_prob=0.1, segments=None, memory_budget=None):
    """Isolated-unit training, as Sheet04 trains by file name (Sheet04.py:116-124): sequence i is one instance of the unit
    ``unit_of_sequence[i]``.  ``sequences``: CUDA float32 or float64 ``[frames, D]`` with ``segments``, or a list of
    per-sequence tensors.  ``n_states``: one integer or ``{unit: states}``.

    The first Gaussians are the means and variances of a hard alignment: ``init_alignments`` (one local state per frame and
    sequence -- the ``*initStates.npy`` Sheet04 loads and then ignores) or the uniform left-to-right split.  Then ``iters``
    times: ``method="baum-welch"`` runs ``forward_backward`` on every sequence under its unit's model, ``gauss_stats`` on the
    posteriors and the M-step (S102); ``"viterbi"`` decodes every sequence and takes the statistics of the hard alignment
    instead.  Transitions start as ``HmmSet.left_to_right(self_prob, next_prob)`` and are re-estimated from the summed edge
    posteriors (or counts).  A Gaussian fed less than ``min_occupancy`` keeps its parameters (the first ones: mean 0,
    variance 1).

    -> ``(HmmSet, logliks)``: ``logliks[k]`` is the summed log-likelihood (Viterbi score) of the sequences under the
    parameters iteration k started from."""
    who = "fit"
    x, seg = _rows(sequences, who, "sequences")
    if seg is not None and segments is not None:
        raise ValueError("%s: segments comes with one tensor; a list carries its own" % who)
    if seg is None:
        seg = np.array([0, int(x.shape[0])], dtype=np.int64) if segments is None else check_segments(segments, int(x.shape[0]), who)
    if (np.diff(seg) < 1).any():
        raise ValueError("%s: every sequence must hold at least one frame" % who)
    lengths, n_seqs, d = np.diff(seg), len(seg) - 1, int(x.shape[1])
    names, counts = check_fit_args(n_seqs, unit_of_sequence, n_states, init_alignments, lengths, iters, method, var_floor, min_occupancy,
                                   self_prob, next_prob)
    firsts = np.concatenate([[0], np.cumsum(counts)])
    g = int(firsts[-1])
    unit_of = np.array([names.index(nm) for nm in unit_of_sequence])
    align = np.empty(int(seg[-1]), dtype=np.int32)
    for i in range(n_seqs):
        local = uniform_alignment(lengths[i], counts[unit_of[i]]) if init_alignments is None else np.asarray(init_alignments[i])
        align[seg[i]:seg[i + 1]] = firsts[unit_of[i]] + local
    means, variances = mstep_gaussians(gauss_stats(x, g, align=align).cpu().numpy(), np.zeros((g, d)), np.ones((g, d)), var_floor,
                                       min_occupancy)
    units = [HmmSet.left_to_right(nm, int(firsts[u]), counts[u], self_prob, next_prob) for u, nm in enumerate(names)]
    jobs = np.array([(i, unit_of[i], 1) for i in range(n_seqs)], dtype=np.int32)
    budget = MEMORY_BUDGET_BYTES if memory_budget is None else int(memory_budget)
    logliks = []
    for _ in range(int(iters)):
        hs = _checked_set(who, means, variances, units)
        models = [hs.compose([nm]) for nm in names]
        logb = emissions(x, hs)
        xi_sum = [np.zeros((c, c)) for c in counts]
        start_sum, exit_sum = [np.zeros(c) for c in counts], [np.zeros(c) for c in counts]
        total = 0.0
        if method == "baum-welch":
            stats = np.zeros((g, 1 + 2 * d))
            pk = _Packed(models, g, x.device, who)
            for lo, hi, gamma, gamma_off, xi_off, xi, ll, _st in _fb_rounds(who, logb, seg, pk, jobs, budget):
                stats = stats + _stats_call(x, g, 0, gamma, contributions(models, seg, jobs[lo:hi], gamma_off, g), None).cpu().numpy()
                n_of = np.array([counts[unit_of[k]] for k in range(lo, hi)], dtype=np.int64)
                first_rows = np.concatenate([gamma_off[k - lo] + np.arange(n_of[k - lo]) for k in range(lo, hi)])
                last_rows = np.concatenate([gamma_off[k - lo + 1] - n_of[k - lo] + np.arange(n_of[k - lo]) for k in range(lo, hi)])
                ends = gamma[torch.as_tensor(np.concatenate([first_rows, last_rows])).to(x.device)].cpu().numpy()
                at = np.concatenate([[0], np.cumsum(n_of)])
                for k in range(lo, hi):  # in job order
                    u, a0, a1 = unit_of[k], at[k - lo], at[k - lo + 1]
                    xi_sum[u] = xi_sum[u] + _dense_xi(models[u], xi[xi_off[k - lo]:xi_off[k - lo + 1]])
                    start_sum[u], exit_sum[u] = start_sum[u] + ends[a0:a1], exit_sum[u] + ends[at[-1] + a0:at[-1] + a1]
                    total = total + ll[k - lo]
        else:
            scores, status, paths = viterbi(logb, models, jobs, segments=seg, memory_budget=budget)
            align = np.full(int(seg[-1]), -1, dtype=np.int32)
            for k in range(n_seqs):  # in job order
                total = total + scores[k]
                if status[k] != STATUS_OK:
                    continue
                u, p = unit_of[k], paths[k]
                align[seg[k]:seg[k + 1]] = models[u].emit[p]
                np.add.at(xi_sum[u], (p[:-1], p[1:]), 1.0)
                start_sum[u][p[0]] += 1.0
                exit_sum[u][p[-1]] += 1.0
            stats = gauss_stats(x, g, align=align).cpu().numpy()
        logliks.append(float(total))
        means, variances = mstep_gaussians(stats, means, variances, var_floor, min_occupancy)
        units = [mstep_unit(units[u], xi_sum[u], start_sum[u], exit_sum[u]) for u in range(len(names))]
    return _checked_set(who, means, variances, units), logliks


def _checked_set(who, means, variances, units):
    if not (np.isfinite(variances).all() and (variances > 0).all()):
        gi = int(np.argwhere(~(np.isfinite(variances) & (variances > 0)))[0][0])
        raise ValueError("%s: the variance of Gaussian %d is not positive and finite; raise var_floor" % (who, gi))
    return HmmSet(means, variances, units)


def save_hmmset(hmmset, path, **extra):
    """An ``HmmSet`` (and ``extra`` arrays) as one ``.npz``."""
    with open(path, "wb") as f:
        np.savez(f, means=hmmset.means, variances=hmmset.variances, names=np.array(hmmset.names, dtype=np.str_),
                 firsts=np.array([u.first for u in hmmset.units], dtype=np.int64),
                 n_states=np.array([u.n_states for u in hmmset.units], dtype=np.int64),
                 log_pi=np.concatenate([u.log_pi for u in hmmset.units] or [np.zeros(0)]),
                 log_a=np.concatenate([u.log_a.ravel() for u in hmmset.units] or [np.zeros(0)]),
                 exit_logp=np.concatenate([u.exit_logp for u in hmmset.units] or [np.zeros(0)]), **extra)


def load_hmmset(z):
    """The ``HmmSet`` of an open ``.npz`` that ``save_hmmset`` wrote."""
    hs = HmmSet(z["means"], z["variances"])
    at, at2 = 0, 0
    for nm, first, n in zip(z["names"], z["firsts"], z["n_states"]):
        n = int(n)
        hs.add_unit(Unit(str(nm), int(first), z["log_pi"][at:at + n], z["log_a"][at2:at2 + n * n].reshape(n, n), z["exit_logp"][at:at + n]))
        at, at2 = at + n, at2 + n * n
    return hs


class HmmSegmenter(object):
    """Sheet04 from unit sequences to segmented videos: ``fit`` trains the units (``hmm.fit``), ``segment`` scores every video
    against every grammar and decodes (``hmm.segment``), ``score`` is the mean over frames against given labels."""

    def __init__(self):
        self.hmmset = self.grammars = self.logliks = None

    def fit(self, sequences, unit_of_sequence, n_states, grammars=None, **fit_kw):
        """``hmm.fit`` with ``fit_kw``; ``grammars`` (a list of unit-name sequences) are kept for ``segment``.  -> self."""
        self.hmmset, self.logliks = fit(sequences, unit_of_sequence, n_states, **fit_kw)
        self.grammars = None if grammars is None else [list(g) for g in grammars]
        return self

    def _grammars(self, grammars, who):
        if self.hmmset is None:
            raise ValueError("%s: the model is not fitted" % who)
        grammars = self.grammars if grammars is None else grammars
        if not grammars:
            raise ValueError("%s: no grammars: pass them here or to fit" % who)
        return grammars

    def segment(self, features, grammars=None, decode="best", segments=None):
        """-> ``Segmentation`` of the videos under the fitted units."""
        return segment(features, self.hmmset, self._grammars(grammars, "HmmSegmenter.segment"), decode=decode, segments=segments)

    def score(self, features, true_units, grammars=None, segments=None):
        """The mean over frames of the best grammar's decoded units against ``true_units``: per video one sequence of unit
        names or of unit indices of the fitted set."""
        out = self.segment(features, self._grammars(grammars, "HmmSegmenter.score"), "best", segments)
        truth = [np.array([self.hmmset.unit_index(u) if isinstance(u, str) else int(u) for u in t]) for t in true_units]
        if len(truth) != len(out.best):
            raise ValueError("HmmSegmenter.score: %d videos but %d label sequences" % (len(out.best), len(truth)))
        return mean_over_frames([out.units(v) for v in range(len(truth))], truth)

    def save(self, path):
        if self.hmmset is None:
            raise ValueError("HmmSegmenter.save: the model is not fitted")
        gr = self.grammars or []
        save_hmmset(self.hmmset, path, logliks=np.asarray(self.logliks if self.logliks is not None else [], dtype=np.float64),
                    grammar_len=np.array([len(g) for g in gr], dtype=np.int64),
                    grammar_units=np.array([u for g in gr for u in g], dtype=np.str_))

    @classmethod
    def load(cls, path):
        m = cls()
        with np.load(path) as z:
            m.hmmset = load_hmmset(z)
            m.logliks = [float(v) for v in z["logliks"]]
            flat, at, m.grammars = [str(u) for u in z["grammar_units"]], 0, []
            for n in z["grammar_len"]:
                m.grammars.append(flat[at:at + int(n)])
                at += int(n)
            m.grammars = m.grammars or None
        return m
