"""Packed VGG-16 stream model on MI355X: host wrapper over ``va_vgg16_*`` (include/va.h).

This is the object the reference obtains from ``models.vgg16(pretrained=True)`` plus
``__swapClassifier__`` (and ``__copyFirstLayer__`` for the temporal stream):
Sheet03/spatialModel.py:110-113,136-152; Sheet03/temporalModel.py:122-126,149-181.
"""
import ctypes
import types

import torch

from . import _ffi

_ws_cache = {}


def _workspace(nbytes, device, slot=0):
    """Grow-only workspace per (device, slot); models that may run concurrently use different slots."""
    key = (device.index, "vgg", slot)
    t = _ws_cache.get(key)
    if t is None or t.numel() < nbytes:
        _ws_cache[key] = t = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return t


def release_workspaces():
    _ws_cache.clear()


def copy_first_layer(w_rgb, n_in):
    """``__copyFirstLayer__`` (Sheet03/temporalModel.py:149-162) on the device: mean of the three RGB
    input-channel slices of ``w_rgb [Cout,3,3,3]`` replicated over ``n_in`` input channels."""
    if not w_rgb.is_cuda or w_rgb.dtype != torch.float32 or w_rgb.dim() != 4 or tuple(w_rgb.shape[1:]) != (3, 3, 3):
        raise ValueError("copy_first_layer: w_rgb must be a CUDA float32 tensor [Cout,3,3,3]")
    w_rgb = w_rgb.contiguous()
    out = torch.empty((w_rgb.shape[0], n_in, 3, 3), dtype=torch.float32, device=w_rgb.device)
    _ffi.check(_ffi.lib().va_copy_first_layer(_ffi.ctx(w_rgb.device.index), _ffi.ptr(w_rgb), w_rgb.shape[0], n_in,
                                              _ffi.ptr(out), _ffi.stream_ptr(w_rgb.device)))
    return out


class Vgg16Stream(object):
    """VGG-16 'D' features + Linear(25088,4096)/ReLU/Linear(4096,4096)/ReLU/Linear(4096,D)/ReLU/
    Linear(D,nClasses), weights packed once for the gfx950 kernels."""

    def __init__(self, conv_w, conv_b, fc_w, fc_b, n_classes, desc_dim, in_mean=None, in_std=None, device=None,
                 ws_slot=0, dtype="f32"):
        """``dtype``: "f32" (exact fp32 MFMA: the parity configuration) or "bf16" (bf16 conv stack with fp32
        accumulation and fp32 classifier: BASELINE config 5, class scores deviate at the 1e-2 level)."""
        if dtype not in ("f32", "bf16"):
            raise ValueError("Vgg16Stream: dtype must be 'f32' or 'bf16'")
        self.dtype = dtype
        if len(conv_w) != 13 or len(conv_b) != 13 or len(fc_w) != 4 or len(fc_b) != 4:
            raise ValueError("Vgg16Stream: need 13 conv and 4 fc weight/bias tensors")
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.device = dev
        self.ws_slot = ws_slot
        self.c_in = int(conv_w[0].shape[1])
        self.n_classes = int(n_classes)
        self.desc_dim = int(desc_dim)
        cin = self.c_in
        for i, (w, b) in enumerate(zip(conv_w, conv_b)):
            co = _ffi_conv_cout(i)
            if tuple(w.shape) != (co, cin, 3, 3) or tuple(b.shape) != (co,):
                raise ValueError("Vgg16Stream: conv layer %d has shape %s / %s, expected %s / %s"
                                 % (i, tuple(w.shape), tuple(b.shape), (co, cin, 3, 3), (co,)))
            cin = co
        fshapes = [(4096, 512 * 7 * 7), (4096, 4096), (self.desc_dim, 4096), (self.n_classes, self.desc_dim)]
        for i, (w, b) in enumerate(zip(fc_w, fc_b)):
            if tuple(w.shape) != fshapes[i] or tuple(b.shape) != (fshapes[i][0],):
                raise ValueError("Vgg16Stream: fc layer %d has shape %s, expected %s" % (i, tuple(w.shape), fshapes[i]))
        keep = []

        def dev_f32(t):
            t = t.to(device=dev, dtype=torch.float32).contiguous()
            keep.append(t)
            return t.data_ptr()

        arr = ctypes.c_void_p * 13
        arr4 = ctypes.c_void_p * 4
        cw = arr(*[dev_f32(t) for t in conv_w])
        cb = arr(*[dev_f32(t) for t in conv_b])
        fw = arr4(*[dev_f32(t) for t in fc_w])
        fb = arr4(*[dev_f32(t) for t in fc_b])
        mean = std = None
        if in_mean is not None and in_std is not None:
            if len(in_mean) != self.c_in or len(in_std) != self.c_in:
                raise ValueError("Vgg16Stream: in_mean/in_std need %d entries" % self.c_in)
            mean = (ctypes.c_float * self.c_in)(*[float(v) for v in in_mean])
            std = (ctypes.c_float * self.c_in)(*[float(v) for v in in_std])
        h = ctypes.c_void_p()
        with torch.cuda.device(dev):
            _ffi.check(_ffi.lib().va_vgg16_create(_ffi.ctx(dev.index), self.c_in, self.n_classes, self.desc_dim,
                                                  1 if dtype == "bf16" else 0,
                                                  cw, cb, fw, fb, mean, std, _ffi.stream_ptr(self.device), ctypes.byref(h)))
        self._h = h
        del keep

    def _on_my_device(self, t, who):
        """The packed weights, the va_ctx and the stream handed over all belong to ``self.device``."""
        if t.device != self.device:
            raise ValueError("Vgg16Stream.%s: tensor is on %s, the model on %s" % (who, t.device, self.device))

    def set_option(self, option, value):
        """``va_vgg16_set_option``: the explicit A/B and test switches of this handle (include/va.h)."""
        _ffi.check(_ffi.lib().va_vgg16_set_option(self._h, int(option), int(value)))

    def close(self):
        if getattr(self, "_h", None):
            _ffi.lib().va_vgg16_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def forward(self, x, want_feat=False):
        """x: CUDA float32 (already normalised) or uint8 ``[B,C,224,224]`` NCHW.
        Returns (feat [B,512,7,7] or None, descriptor [B,D], logits [B,nClasses])."""
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError("Vgg16Stream.forward: x must be a CUDA tensor")
        if x.dim() != 4 or tuple(x.shape[1:]) != (self.c_in, 224, 224):
            raise ValueError("Vgg16Stream.forward: x must be [B,%d,224,224], got %s" % (self.c_in, tuple(x.shape)))
        if x.dtype not in (torch.float32, torch.uint8):
            raise ValueError("Vgg16Stream.forward: x must be float32 or uint8")
        self._on_my_device(x, "forward")
        x = x.contiguous()
        B = x.shape[0]
        L = _ffi.lib()
        nbytes = L.va_vgg16_workspace_bytes(self._h, B)
        ws = _workspace(nbytes, x.device, self.ws_slot)
        feat = torch.empty((B, 512, 7, 7), dtype=torch.float32, device=x.device) if want_feat else None
        desc = torch.empty((B, self.desc_dim), dtype=torch.float32, device=x.device)
        logits = torch.empty((B, self.n_classes), dtype=torch.float32, device=x.device)
        _ffi.check(L.va_vgg16_forward(self._h, _ffi.ptr(x), int(x.dtype == torch.uint8), B, _ffi.ptr(feat),
                                      _ffi.ptr(desc), _ffi.ptr(logits), _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr(self.device)))
        return feat, desc, logits

    VIEW_CHUNK = 320  # images per forward call of forward_views (ten views x the configured batch of 32)

    def forward_views(self, x):
        """x: CUDA float32 (normalised) or uint8 ``[B,V,C,224,224]``, V views of every clip (ten-crop evaluation,
        DESIGN.md S10).  Returns (desc [B,D], logits [B,nClasses], desc_views [B,V,D], logits_views [B,V,nClasses]):
        the per-view outputs of ``forward`` and their ``view_mean``.

        The B*V images run in chunks of whole clips of at most ``VIEW_CHUNK`` images: the bf16 conv stack refuses more
        than about 334 images at 224x224 (32-bit buffer offsets), fp32 224x224x64 activations pass 2^31 elements at 669
        images, and 320 is ten views of the configured batch of 32.  A chunk's outputs are the rows ``forward`` gives for
        that chunk alone."""
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError("Vgg16Stream.forward_views: x must be a CUDA tensor")
        if x.dim() != 5 or tuple(x.shape[2:]) != (self.c_in, 224, 224):
            raise ValueError("Vgg16Stream.forward_views: x must be [B,V,%d,224,224], got %s" % (self.c_in, tuple(x.shape)))
        if x.dtype not in (torch.float32, torch.uint8):
            raise ValueError("Vgg16Stream.forward_views: x must be float32 or uint8")
        self._on_my_device(x, "forward_views")
        B, V = int(x.shape[0]), int(x.shape[1])
        if B < 1 or V < 1 or V > self.VIEW_CHUNK:
            raise ValueError("Vgg16Stream.forward_views: need 1..%d views and at least one clip, got B=%d V=%d"
                             % (self.VIEW_CHUNK, B, V))
        x = x.contiguous().view(B * V, self.c_in, 224, 224)
        per = (self.VIEW_CHUNK // V) * V
        L = _ffi.lib()
        ws = _workspace(L.va_vgg16_workspace_bytes(self._h, min(per, B * V)), x.device, self.ws_slot)
        desc_v = torch.empty((B, V, self.desc_dim), dtype=torch.float32, device=x.device)
        logits_v = torch.empty((B, V, self.n_classes), dtype=torch.float32, device=x.device)
        dflat, lflat = desc_v.view(B * V, -1), logits_v.view(B * V, -1)
        for i0 in range(0, B * V, per):
            n = min(per, B * V - i0)
            _ffi.check(L.va_vgg16_forward(self._h, _ffi.ptr(x[i0:i0 + n]), int(x.dtype == torch.uint8), n, None,
                                          _ffi.ptr(dflat[i0:i0 + n]), _ffi.ptr(lflat[i0:i0 + n]), _ffi.ptr(ws), ws.numel(),
                                          _ffi.stream_ptr(self.device)))
        return view_mean(desc_v), view_mean(logits_v), desc_v, logits_v

    def features(self, x):
        """``self.features(ip)`` of the reference (Sheet03/spatialModel.py:212): [B,C,224,224] -> [B,512,7,7]."""
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError("Vgg16Stream.features: x must be a CUDA tensor")
        if x.dim() != 4 or tuple(x.shape[1:]) != (self.c_in, 224, 224) or x.dtype not in (torch.float32, torch.uint8):
            raise ValueError("Vgg16Stream.features: x must be float32/uint8 [B,%d,224,224]" % self.c_in)
        self._on_my_device(x, "features")
        x = x.contiguous()
        B = x.shape[0]
        L = _ffi.lib()
        ws = _workspace(L.va_vgg16_workspace_bytes(self._h, B), x.device, self.ws_slot)
        feat = torch.empty((B, 512, 7, 7), dtype=torch.float32, device=x.device)
        _ffi.check(L.va_vgg16_forward(self._h, _ffi.ptr(x), int(x.dtype == torch.uint8), B, _ffi.ptr(feat), None, None,
                                      _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr(self.device)))
        return feat

    def first_layer(self, x, staged, out):
        """The model's first stage alone (``va_vgg16_first_layer``, a testing entry point): the input conversion, where the
        path has one, into ``staged``, then conv layer 0 into ``out``, through the function ``forward`` runs first.
        x: CUDA float32 / uint8 ``[B,C,224,224]`` (any alignment of its element type); out: NHWC ``[B,224,224,64]`` of the
        model's dtype; staged: ``[B,224*224,c_in_pad]`` float32 (fp32 models) or ``[B,224*224,64]`` bfloat16.  Returns the
        names of the kernel instantiations that ran.  Enqueued on the current stream; nothing is synchronised."""
        tdt = torch.bfloat16 if self.dtype == "bf16" else torch.float32
        if (not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 4 or tuple(x.shape[1:]) != (self.c_in, 224, 224)
                or x.dtype not in (torch.float32, torch.uint8) or not x.is_contiguous()):
            raise ValueError("Vgg16Stream.first_layer: x must be a contiguous CUDA float32/uint8 [B,%d,224,224]" % self.c_in)
        B = int(x.shape[0])
        cpad = 64 if self.dtype == "bf16" else (self.c_in + 15) // 16 * 16
        for name, t, shape in (("staged", staged, (B, 224 * 224, cpad)), ("out", out, (B, 224, 224, 64))):
            if (not isinstance(t, torch.Tensor) or t.dtype != tdt or tuple(t.shape) != shape or not t.is_contiguous()):
                raise ValueError("Vgg16Stream.first_layer: %s must be a contiguous %s tensor %s" % (name, tdt, shape))
            self._on_my_device(t, "first_layer")
        self._on_my_device(x, "first_layer")
        info = ctypes.create_string_buffer(160)
        _ffi.check(_ffi.lib().va_vgg16_first_layer(self._h, _ffi.ptr(x), int(x.dtype == torch.uint8), B, _ffi.ptr(staged),
                                                   _ffi.ptr(out), info, len(info), _ffi.stream_ptr(self.device)))
        return info.value.decode()

    def classify(self, feat):
        """The classifierList traversal (Sheet03/spatialModel.py:213-218): feat [B,512,7,7] ->
        (featureVectors [B,D] = output of module 8, logits [B,nClasses] = output of module 9)."""
        if not isinstance(feat, torch.Tensor) or not feat.is_cuda or feat.dtype != torch.float32:
            raise ValueError("Vgg16Stream.classify: feat must be a CUDA float32 tensor")
        if feat.dim() != 4 or tuple(feat.shape[1:]) != (512, 7, 7):
            raise ValueError("Vgg16Stream.classify: feat must be [B,512,7,7]")
        self._on_my_device(feat, "classify")
        feat = feat.contiguous()
        B = feat.shape[0]
        L = _ffi.lib()
        ws = _workspace(L.va_vgg16_workspace_bytes(self._h, B), feat.device, self.ws_slot)
        desc = torch.empty((B, self.desc_dim), dtype=torch.float32, device=feat.device)
        logits = torch.empty((B, self.n_classes), dtype=torch.float32, device=feat.device)
        _ffi.check(L.va_vgg16_classify(self._h, _ffi.ptr(feat), B, _ffi.ptr(desc), _ffi.ptr(logits), _ffi.ptr(ws),
                                       ws.numel(), _ffi.stream_ptr(self.device)))
        return desc, logits


    def classifier_list(self):
        """The indexable ``self.classifierList`` of the reference (``list(self.model.classifier)``: Linear, ReLU, Dropout,
        Linear, ReLU, Dropout, Linear, ReLU, Dropout, Linear; Sheet03/spatialModel.py:128-129) as ten callables, so that
        the reference's own traversal runs unchanged over the fused kernels:

            op = self.features(ip); op = op.view(op.size(0), -1)
            for cl in self.classifierList[:9]: op = cl(op)      # -> featureVectors [B, D]
            for cl in self.classifierList[9:]: op = cl(op)      # -> class scores   [B, nClasses]

        Stage 0 runs the whole classifier (``va_vgg16_classify``) on the flattened features, stages 1..7 hand its result
        on, stage 8 returns the descriptor tensor, stage 9 returns the scores that belong to exactly that tensor (any
        other input raises ``ValueError``: the stages are one fused operator, not ten independent modules)."""
        return [_ClassifierStage(self, i) for i in range(10)]

    # ---- training (fp32 models only) ----

    def train_init(self):
        """Allocate and zero the momentum buffers (``tch.optim.SGD(..., momentum=...)``, Sheet03/spatialModel.py:116)."""
        _ffi.check(_ffi.lib().va_vgg16_train_init(self._h, _ffi.stream_ptr(self.device)))
        self._train_ready = True

    def set_solver(self, solver):
        """``va_vgg16_set_solver``: weight decay, bias multipliers, the three dropout ratios and the frozen
        layers that every form of the step and ``train_apply`` read from now on.  A stream whose solver was never set
        behaves as with ``Solver()``.  ValueError (nothing changes) for anything but a ``Solver``, and on a bf16 model."""
        if not isinstance(solver, Solver):
            raise ValueError("Vgg16Stream.set_solver: need a vgg.Solver, got %r" % (solver,))
        s = solver.to_struct()
        _ffi.check(_ffi.lib().va_vgg16_set_solver(self._h, ctypes.byref(s)))

    @property
    def solver(self):
        """The stream's solver state (``va_vgg16_get_solver``) as a ``Solver``."""
        s = _ffi.SolverParams()
        _ffi.check(_ffi.lib().va_vgg16_get_solver(self._h, ctypes.byref(s)))
        return Solver.from_struct(s)

    def train_step(self, x, labels, lr, momentum, dropout_seed):
        """One iteration of the batch loop of ``train()`` (Sheet03/spatialModel.py:165-182): forward in train
        mode, mean cross-entropy, backward, SGD update.  Returns (stats, descriptors): ``stats`` is a CUDA
        float32 ``[2]`` = (loss, number of arg-max hits) of the forward pass, ``descriptors`` ``[B,D]`` the
        train-mode feature tap; nothing synchronises the host."""
        p = self._train_batch("train_step", x, labels)
        _ffi.check(_ffi.lib().va_vgg16_train_step(self._h, _ffi.ptr(p.x), p.is_u8, _ffi.ptr(p.labels), p.B, float(lr),
                                                  float(momentum), int(dropout_seed) & 0xFFFFFFFFFFFFFFFF, _ffi.ptr(p.desc),
                                                  _ffi.ptr(p.stats), _ffi.ptr(p.ws), p.ws.numel(), _ffi.stream_ptr(self.device)))
        return p.stats, p.desc

    # what differs between the four wrappers in the checks they share: the letters of x's first dimension, the smallest k (None:
    # no k, every image is its own video), the two texts about labels (None: check_tasks or the kernel speaks) and the text
    # for a batch size the library refuses
    _TRAIN_TEXTS = {
        "train_step": ("B", None, None, "labels must be [B]", "batch %(B)d unsupported (1..64, fp32 model)"),
        "train_step_consensus": ("n*k", 1, "labels must be a tensor [n]", "labels must be [%(n)d], one per video",
                                 "%(n)d videos x %(k)d snippets unsupported (n*k in 1..64, fp32 model)"),
        "train_step_multitask": ("n*k", 1, None, None, "%(n)d videos x %(k)d snippets unsupported (n*k in 1..64, fp32 model)"),
        "train_accumulate": ("B", 0, "labels must be a tensor [%(n)d]", "labels must be [%(n)d]",
                             "%(B)d images unsupported (1..64 per micro-batch, fp32 model)"),
    }

    def _train_batch(self, name, x, labels, k=None, tasks=None, heads=None, multitask=False, init_first=True):
        """What every form of the training step does before its ABI call: the lazy ``train_init``, the checks on ``x``, the
        whole-number-of-videos rule (``k = 0``: images, where ``name`` allows it), labels (``multitask``: and tasks, against
        ``heads``) checked and moved to the device, the workspace, and the outputs.  -> a namespace: ``x`` (contiguous), ``is_u8``, ``labels``, ``tasks``,
        ``heads`` (a list, or None), ``B``, ``n``, ``k``, ``ws``, ``stats`` f32 ``[2]`` or ``[2+2H]``, ``desc`` f32 ``[B,D]``.
        ``init_first=False``: ``train_init`` runs after the checks instead (``train_accumulate`` refuses bad arguments on a
        model that has never trained without allocating its momentum buffers)."""
        who = "Vgg16Stream." + name
        dims, k_min, not_a_tensor, bad_shape, unsupported = self._TRAIN_TEXTS[name]
        if init_first and not getattr(self, "_train_ready", False):
            self.train_init()
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype not in (torch.float32, torch.uint8):
            raise ValueError("%s: x must be a CUDA float32/uint8 tensor" % who)
        if x.dim() != 4 or tuple(x.shape[1:]) != (self.c_in, 224, 224):
            raise ValueError("%s: x must be [%s,%d,224,224], got %s" % (who, dims, self.c_in, tuple(x.shape)))
        self._on_my_device(x, name)
        if multitask:
            check_heads(heads, self.n_classes, who)
            heads = [int(h) for h in heads]
        B = n = int(x.shape[0])
        if k_min is not None:
            k = int(k)
            if k < k_min or B < 1 or B % max(k, 1):
                raise ValueError("%s: %d images are not a whole number of videos of k=%d snippets" % (who, B, k))
            n = B // max(k, 1)
        sizes = dict(B=B, n=n, k=k)
        if multitask:
            labels, tasks = check_tasks(labels, tasks, heads, n, who)
            tasks = tasks.to(device=x.device, dtype=torch.int32).contiguous()
        else:
            _check_labels(labels, self.n_classes, who)
            if not_a_tensor is not None and not isinstance(labels, torch.Tensor):
                raise ValueError("%s: %s" % (who, not_a_tensor % sizes))
        labels = labels.to(device=x.device, dtype=torch.int64).contiguous()
        if bad_shape is not None and (labels.dim() != 1 or labels.shape[0] != n):
            raise ValueError("%s: %s" % (who, bad_shape % sizes))
        if not init_first and not getattr(self, "_train_ready", False):
            self.train_init()
        nbytes = _ffi.lib().va_vgg16_train_workspace_bytes(self._h, B)
        if nbytes == 0:
            raise ValueError("%s: %s" % (who, unsupported % sizes))
        return types.SimpleNamespace(
            x=x.contiguous(), is_u8=int(x.dtype == torch.uint8), labels=labels, tasks=tasks, heads=heads, B=B, n=n, k=k,
            ws=_workspace(nbytes, x.device, ("train", self.ws_slot)),
            stats=torch.empty(2 + 2 * len(heads) if heads else 2, dtype=torch.float32, device=x.device),
            desc=torch.empty((B, self.desc_dim), dtype=torch.float32, device=x.device))

    def train_step_consensus(self, x, labels, k, lr, momentum, dropout_seed):
        """``train_step`` with the loss on the consensus of each video's ``k`` snippets (TSN's segmental
        consensus): x ``[n*k,C,224,224]``, video-major, labels ``[n]``, ``n*k <= 64``.  The k snippets' class scores are
        averaged (in snippet order), the mean cross-entropy of the n averages is the loss, and every snippet receives
        1/k of its video's gradient.  Returns (stats, descriptors): ``stats`` = (loss, arg-max hits of the averaged
        scores), ``descriptors`` ``[n*k,D]``.  ``k = 1`` is ``train_step`` bit for bit."""
        p = self._train_batch("train_step_consensus", x, labels, k)
        _ffi.check(_ffi.lib().va_vgg16_train_step_consensus(
            self._h, _ffi.ptr(p.x), p.is_u8, _ffi.ptr(p.labels), p.n, p.k, float(lr), float(momentum),
            int(dropout_seed) & 0xFFFFFFFFFFFFFFFF, _ffi.ptr(p.desc), _ffi.ptr(p.stats), _ffi.ptr(p.ws), p.ws.numel(),
            _ffi.stream_ptr(self.device)))
        return p.stats, p.desc

    def train_step_multitask(self, x, labels, tasks, heads, k, lr, momentum, dropout_seed):
        """``train_step_consensus`` with one loss per dataset (multi-task learning, Sheet03/notes.txt:88-96):
        the model's ``n_classes`` outputs are the concatenated heads ``heads = (C_0, ..., C_{H-1})``, 1 to 8 of them; x
        ``[n*k,C,224,224]``, video-major, ``n*k <= 64``; ``tasks [n]`` names each video's head and ``labels [n]`` are local
        to it (``0 <= label < C_task``).  Each head's loss is the consensus loss of its own videos on its own outputs; the
        step descends their sum, and a head without a video in the batch moves by its momentum alone.  Returns (stats,
        descriptors): ``stats`` f32 ``[2+2H]`` = (loss, hits, loss of every head, hits of every head), ``descriptors``
        ``[n*k,D]``.  One head is ``train_step_consensus`` bit for bit.  Labels and tasks still on the host are checked here
        (ValueError); on the device a bad row gives a NaN loss."""
        p = self._train_batch("train_step_multitask", x, labels, k, tasks, heads, multitask=True)
        H = len(p.heads)
        _ffi.check(_ffi.lib().va_vgg16_train_step_multitask(
            self._h, _ffi.ptr(p.x), p.is_u8, _ffi.ptr(p.labels), _ffi.ptr(p.tasks), p.n, p.k, H, (ctypes.c_int * H)(*p.heads),
            float(lr), float(momentum), int(dropout_seed) & 0xFFFFFFFFFFFFFFFF, _ffi.ptr(p.desc), _ffi.ptr(p.stats),
            _ffi.ptr(p.ws), p.ws.numel(), _ffi.stream_ptr(self.device)))
        return p.stats, p.desc

    # ---- the step in two halves: accumulate the gradient, then apply it ----

    def grad(self):
        """The flat float32 gradient buffer of ``train_accumulate`` / ``train_apply`` (``va_vgg16_train_grad_floats``, about
        540 MB), allocated on first use and owned by this object.  ``grad_layout()`` names its 34 segments."""
        g = getattr(self, "_grad", None)
        if g is None:
            n = int(_ffi.lib().va_vgg16_train_grad_floats(self._h))
            if n == 0:
                raise ValueError("Vgg16Stream.grad: training is fp32 only")
            self._grad = g = torch.empty(n, dtype=torch.float32, device=self.device)
        return g

    def grad_layout(self):
        """-> (offsets, counts), 34 ints each, in floats: conv 0..12 as (weight, bias), then fc 0..3 as (weight, bias), every
        tensor in the layout of its parameter (conv weights packed ``[cout][9][cin_pad]``, FC1 in NHWC-flatten order)."""
        off, cnt = (ctypes.c_size_t * 34)(), (ctypes.c_size_t * 34)()
        _ffi.check(_ffi.lib().va_vgg16_train_grad_layout(self._h, off, cnt))
        return [int(v) for v in off], [int(v) for v in cnt]

    def train_accumulate(self, x, labels, *, k=0, tasks=None, heads=None, scales=None, first, dropout_seed):
        """Forward and backward of one micro-batch into ``grad()``; weights and momentum buffers stay as they are
        (``va_vgg16_train_accumulate``).  ``k = 0``: ``train_step``'s loss on the images of x; ``k >= 1``:
        ``train_step_consensus``'s on ``n = len(x) / k`` videos; ``tasks`` and ``heads``: ``train_step_multitask``'s.
        ``scales``: None (1), a number, or with heads one number per head: the gradient at the logits is multiplied by its
        head's scale, ``n_micro / n_full`` for a micro-batch's share of a full batch's mean.  ``first``: True stores the
        gradient, False adds it to what ``grad()`` holds.  Returns (stats, descriptors) as the fused steps do; the loss
        in ``stats`` is the micro-batch's own mean, not scaled."""
        who = "Vgg16Stream.train_accumulate"
        if (tasks is None) != (heads is None):
            raise ValueError("%s: tasks= and heads= go together" % who)
        k = int(k)
        if k < 0 or (tasks is not None and k < 1):
            raise ValueError("%s: k must be >= 0 (>= 1 with tasks=), got %d" % (who, k))
        n_heads = 0
        if heads is not None:
            check_heads(heads, self.n_classes, who)
            n_heads = len(heads)
        scales = check_scales(scales, max(n_heads, 1), who)
        p = self._train_batch("train_accumulate", x, labels, k, tasks, heads, multitask=tasks is not None, init_first=False)
        g = self.grad()
        _ffi.check(_ffi.lib().va_vgg16_train_accumulate(
            self._h, _ffi.ptr(p.x), p.is_u8, _ffi.ptr(p.labels), _ffi.ptr(p.tasks), p.n, p.k, n_heads,
            (ctypes.c_int * n_heads)(*p.heads) if n_heads else None, (ctypes.c_float * len(scales))(*scales), int(bool(first)),
            int(dropout_seed) & 0xFFFFFFFFFFFFFFFF, _ffi.ptr(p.desc), _ffi.ptr(p.stats), _ffi.ptr(g), g.numel(), _ffi.ptr(p.ws),
            p.ws.numel(), _ffi.stream_ptr(self.device)))
        return p.stats, p.desc

    def train_apply(self, lr, momentum, clip_norm=None):
        """The momentum-SGD update of every parameter from ``grad()`` (``va_vgg16_train_apply``):
        ``V = momentum V + c G; W -= lr V`` with the fused step's two fused multiply-adds.  ``clip_norm``: None (no clipping,
        ``c`` absent) or a positive number: ``c = min(1, clip_norm / (|G| + 1e-6))``, ``torch.nn.utils.clip_grad_norm_``'s rule,
        with the norm a float64 sum in a fixed order, all on the device.  Returns the norm as a CUDA float64 ``[1]`` tensor,
        or None without clipping; nothing synchronises the host."""
        who = "Vgg16Stream.train_apply"
        clip = check_clip_norm(clip_norm, who)
        if getattr(self, "_grad", None) is None:
            raise ValueError("%s: nothing was accumulated (call train_accumulate first)" % who)
        if not getattr(self, "_train_ready", False):
            self.train_init()
        L = _ffi.lib()
        g = self._grad
        norm = ws = None
        if clip > 0.0:
            norm = torch.empty(1, dtype=torch.float64, device=self.device)
            ws = _workspace(int(L.va_vgg16_train_apply_workspace_bytes()), self.device, ("train", self.ws_slot))
        _ffi.check(L.va_vgg16_train_apply(self._h, _ffi.ptr(g), g.numel(), float(lr), float(momentum), clip, _ffi.ptr(norm), _ffi.ptr(ws),
                                          ws.numel() if ws is not None else 0, _ffi.stream_ptr(self.device)))
        return norm

    def export_grad(self):
        """-> dict(conv_w, conv_b, fc_w, fc_b) like ``export_state``: the accumulated gradient in the reference's layouts,
        what ``p.grad`` holds after ``loss.backward()`` (``va_vgg16_unpack_grad``)."""
        if getattr(self, "_grad", None) is None:
            raise ValueError("Vgg16Stream.export_grad: nothing was accumulated (call train_accumulate first)")
        cw, cb, fw, fb = self._state_tensors(self.device)
        arr, arr4 = ctypes.c_void_p * 13, ctypes.c_void_p * 4
        _ffi.check(_ffi.lib().va_vgg16_unpack_grad(self._h, _ffi.ptr(self._grad), arr(*[t.data_ptr() for t in cw]),
                                                   arr(*[t.data_ptr() for t in cb]), arr4(*[t.data_ptr() for t in fw]),
                                                   arr4(*[t.data_ptr() for t in fb]), _ffi.stream_ptr(self.device)))
        return dict(conv_w=cw, conv_b=cb, fc_w=fw, fc_b=fb)

    def _state_tensors(self, device):
        cin = self.c_in
        cw, cb = [], []
        for i in range(13):
            co = _ffi_conv_cout(i)
            cw.append(torch.empty((co, cin, 3, 3), dtype=torch.float32, device=device))
            cb.append(torch.empty((co,), dtype=torch.float32, device=device))
            cin = co
        fshapes = [(4096, 512 * 7 * 7), (4096, 4096), (self.desc_dim, 4096), (self.n_classes, self.desc_dim)]
        fw = [torch.empty(sh, dtype=torch.float32, device=device) for sh in fshapes]
        fb = [torch.empty((sh[0],), dtype=torch.float32, device=device) for sh in fshapes]
        return cw, cb, fw, fb

    def export_state(self, momentum=False):
        """-> dict(conv_w, conv_b, fc_w, fc_b) of CUDA tensors in the reference's layouts: the parameters
        (``model.state_dict()``) or, with ``momentum=True``, SGD's momentum buffers."""
        dev = torch.device("cuda", torch.cuda.current_device())
        cw, cb, fw, fb = self._state_tensors(dev)
        arr, arr4 = ctypes.c_void_p * 13, ctypes.c_void_p * 4
        _ffi.check(_ffi.lib().va_vgg16_export_state(self._h, int(bool(momentum)), arr(*[t.data_ptr() for t in cw]),
                                                    arr(*[t.data_ptr() for t in cb]), arr4(*[t.data_ptr() for t in fw]),
                                                    arr4(*[t.data_ptr() for t in fb]), _ffi.stream_ptr(self.device)))
        return dict(conv_w=cw, conv_b=cb, fc_w=fw, fc_b=fb)

    def import_state(self, state, momentum=False):
        """Load parameters (or momentum buffers) from dict(conv_w, conv_b, fc_w, fc_b) in the reference's layouts."""
        if momentum and not getattr(self, "_train_ready", False):
            self.train_init()
        dev = torch.device("cuda", torch.cuda.current_device())
        keep = []

        def p(t):
            t = t.to(device=dev, dtype=torch.float32).contiguous()
            keep.append(t)
            return t.data_ptr()

        ref = self._state_tensors("meta")
        for name, want in zip(("conv_w", "conv_b", "fc_w", "fc_b"), ref):
            got = state[name]
            if len(got) != len(want) or any(tuple(g.shape) != tuple(w.shape) for g, w in zip(got, want)):
                raise ValueError("Vgg16Stream.import_state: %s does not match the model's shapes" % name)
        arr, arr4 = ctypes.c_void_p * 13, ctypes.c_void_p * 4
        _ffi.check(_ffi.lib().va_vgg16_import_state(self._h, int(bool(momentum)), arr(*[p(t) for t in state["conv_w"]]),
                                                    arr(*[p(t) for t in state["conv_b"]]), arr4(*[p(t) for t in state["fc_w"]]),
                                                    arr4(*[p(t) for t in state["fc_b"]]), _ffi.stream_ptr(self.device)))
        torch.cuda.current_stream(self.device).synchronize()  # `keep` must outlive the copies (the model's device, not the thread's current one)
        del keep


def weights_from_state_dict(state_dict):
    """Weights of a torchvision-style VGG-16 state dict as saved by the reference
    (``checkpoint["model"]``, Sheet03/spatialModel.py:256-261; keys carry the ``module.`` prefix of the
    ``nn.DataParallel`` wrapper, ``:133,258``): ``features.{0,2,5,...}.weight/bias`` and
    ``classifier.{0,3,6,9}.weight/bias`` -> dict(conv_w, conv_b, fc_w, fc_b)."""
    sd = {}
    for k, v in state_dict.items():
        sd[k[len("module."):] if k.startswith("module.") else k] = v
    conv_idx = [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]  # Conv2d positions in VGG-16 'D' features
    fc_idx = [0, 3, 6, 9]                                          # Linear positions in the swapped classifier
    try:
        return dict(conv_w=[sd["features.%d.weight" % i] for i in conv_idx],
                    conv_b=[sd["features.%d.bias" % i] for i in conv_idx],
                    fc_w=[sd["classifier.%d.weight" % i] for i in fc_idx],
                    fc_b=[sd["classifier.%d.bias" % i] for i in fc_idx])
    except KeyError as e:
        raise ValueError("weights_from_state_dict: missing key %s (not a VGG-16 'D' + 4-layer classifier state dict)" % e)


CONV_IDX = [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]  # Conv2d positions in VGG-16 'D' features
FC_IDX = [0, 3, 6, 9]                                          # Linear positions in the swapped classifier


def state_dict_from_weights(weights, prefix="module."):
    """dict(conv_w, conv_b, fc_w, fc_b) -> an ordered torchvision-style state dict with the ``module.`` prefix the
    reference's ``nn.DataParallel`` wrapper gives its keys (Sheet03/spatialModel.py:133,258): the inverse of
    ``weights_from_state_dict``; also the order of ``model.parameters()`` (weight, bias per layer)."""
    from collections import OrderedDict
    sd = OrderedDict()
    for i, k in enumerate(CONV_IDX):
        sd["%sfeatures.%d.weight" % (prefix, k)] = weights["conv_w"][i]
        sd["%sfeatures.%d.bias" % (prefix, k)] = weights["conv_b"][i]
    for i, k in enumerate(FC_IDX):
        sd["%sclassifier.%d.weight" % (prefix, k)] = weights["fc_w"][i]
        sd["%sclassifier.%d.bias" % (prefix, k)] = weights["fc_b"][i]
    return sd


class _FusedHead(object):
    """What flows between the stages of ``classifier_list()``: both outputs of the fused classifier."""

    def __init__(self, desc, logits):
        self.desc, self.logits = desc, logits


def classifier_modules(desc_dim, n_classes):
    """The module list ``__swapClassifier__`` builds (Sheet03/spatialModel.py:136-152 = temporalModel.py:165-181), as
    data: what the ten stages of ``classifier_list()`` stand for and what shapes ``fc_w`` / ``fc_b`` must have.  Pinned to
    the reference's own method run on a stub model (tests/golden/reference_model_kats.json)."""
    dims = [(512 * 7 * 7, 4096), (4096, 4096), (4096, desc_dim), (desc_dim, n_classes)]
    mods = []
    for i, (fin, fout) in enumerate(dims):
        mods.append({"type": "Linear", "in_features": fin, "out_features": fout, "bias": True})
        if i < 3:
            mods.append({"type": "ReLU", "inplace": True})
            mods.append({"type": "Dropout", "p": 0.5})
    return mods


class _ClassifierStage(object):
    def __init__(self, stream, index):
        self.stream, self.index = stream, index
        self.module = classifier_modules(stream.desc_dim, stream.n_classes)[index]  # what the reference has at this index

    def __call__(self, op):
        st = self.stream
        if self.index == 0:
            if not isinstance(op, torch.Tensor) or op.dim() != 2 or op.shape[1] != 512 * 7 * 7:
                raise ValueError("classifierList[0]: expected the flattened features [B, 25088]")
            desc, logits = st.classify(op.reshape(op.shape[0], 512, 7, 7))
            return _FusedHead(desc, logits)
        if self.index < 8:
            if not isinstance(op, _FusedHead):
                raise ValueError("classifierList[%d]: apply the stages in order, starting from classifierList[0]" % self.index)
            return op
        if self.index == 8:
            if not isinstance(op, _FusedHead):
                raise ValueError("classifierList[8]: apply the stages in order, starting from classifierList[0]")
            st._head = (op.desc, op.logits)
            return op.desc
        head = getattr(st, "_head", None)
        if head is None or op is not head[0]:
            raise ValueError("classifierList[9]: expected the descriptor tensor classifierList[8] returned")
        return head[1]


def conv3x3_layer(x, w_packed, bias, out, kernel_opt=1, pool=False, linear=False, mask=None, zeros=None):
    """One conv layer through the model's own kernel dispatch (``va_conv3x3_layer``, a testing entry point); returns the
    name of the kernel instantiation that ran.  Layouts are the kernels' own: x NHWC [B][hw][hw][cin_pad] (float32 or
    bfloat16), w_packed [cout][9][cin_pad] of x's dtype, bias float32 [cout], out NHWC [B][hw'][hw'][cout] of x's dtype or
    float32 (bf16 with pool: the fp32-output form), hw' = hw // 2 when pooling; mask float32 shaped like out or None;
    zeros: >= 256 zero bytes on the device (None: allocated here).  kernel_opt is VA_OPT_F32_CONV_KERNEL (fp32) or
    VA_OPT_BF16_VARIANT (bf16).  Enqueued on the current stream; nothing is synchronised."""
    if x.dtype not in (torch.float32, torch.bfloat16) or x.dim() != 4 or x.shape[1] != x.shape[2]:
        raise ValueError("conv3x3_layer: x must be float32 / bfloat16 NHWC [B][hw][hw][cin_pad]")
    B, hw, _, cin_pad = x.shape
    cout = w_packed.shape[0]
    bf = x.dtype == torch.bfloat16
    out_f32 = bf and out.dtype == torch.float32
    hwo = hw // 2 if pool else hw
    tensors = [x, w_packed, bias, out] + ([mask] if mask is not None else [])
    if (w_packed.dtype != x.dtype or tuple(w_packed.shape) != (cout, 9, cin_pad) or bias.dtype != torch.float32
            or tuple(bias.shape) != (cout,) or out.dtype not in (x.dtype, torch.float32)
            or tuple(out.shape) != (B, hwo, hwo, cout) or (mask is not None and (mask.dtype != torch.float32
                                                                                 or mask.shape != out.shape))):
        raise ValueError("conv3x3_layer: w_packed / bias / out / mask do not match x")
    if any(not t.is_cuda or t.device != x.device or not t.is_contiguous() for t in tensors):
        raise ValueError("conv3x3_layer: every tensor must be a contiguous tensor on x's device")
    if zeros is None:
        zeros = torch.zeros(256, dtype=torch.uint8, device=x.device)
    name = ctypes.create_string_buffer(128)
    _ffi.check(_ffi.lib().va_conv3x3_layer(
        _ffi.ctx(x.device.index), 1 if bf else 0, int(kernel_opt), hw, cin_pad, cout, int(bool(pool)), int(bool(linear)),
        int(out_f32), B, _ffi.ptr(x), _ffi.ptr(w_packed), _ffi.ptr(bias), _ffi.ptr(mask), _ffi.ptr(zeros), _ffi.ptr(out),
        name, len(name), _ffi.stream_ptr(x.device)))
    return name.value.decode()


def _f32_cuda(who, ref, **tensors):
    for name, t in tensors.items():
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_cuda or t.device != ref.device or not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous float32 tensor on %s" % (who, name, ref.device))


def train_conv_backward_scratch(B, hw, cin, cin_pad, cout, device=None):
    """(slab, wt, bpart) sizes in floats and the weight-gradient plan of ``train_conv_backward_layer`` (the size query of
    ``va_train_conv_backward_layer``: nothing is launched)."""
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
    need = (ctypes.c_size_t * 3)(0, 0, 0)
    info = ctypes.create_string_buffer(192)
    _ffi.check(_ffi.lib().va_train_conv_backward_layer(
        _ffi.ctx(dev.index), 1, B, hw, cin, cin_pad, cout, None, None, None, None, None, None, 0.0, 0.0, None, None, None, None, None,
        None, need, info, len(info), _ffi.stream_ptr(dev)))
    return tuple(int(v) for v in need), _parse_plan(info.value.decode())


def _parse_plan(text):
    parts = text.split()
    plan = {"wgrad": parts[0]}
    for kv in parts[1:]:
        k, v = kv.split("=", 1)
        plan[k] = v if k == "dgrad" else int(v)
    return plan


def train_conv_backward_layer(dy, x, w_packed, bias, mom_w, mom_b, lr, momentum, cin, dx=None, mask=None, kernel_opt=1, zeros=None,
                              scratch=None):
    """Backward of one conv layer exactly as the training step does it (``va_train_conv_backward_layer``, a testing entry
    point): dy NHWC [B][hw][hw][cout], x NHWC [B][hw][hw][cin_pad], w_packed / mom_w [cout][9][cin_pad], bias / mom_b [cout],
    all float32 on one device; parameters and momentum buffers are updated in place.  dx: NHWC [B][hw][hw][cin] or None
    (no data gradient); mask shaped like dx or None.  scratch: (slab, wt, bpart) float32 tensors or None (allocated here).
    Returns the plan that ran as a dict (wgrad, S, chunk, Mpad, Npad, bgrad_blocks, dgrad)."""
    who = "train_conv_backward_layer"
    if dy.dim() != 4 or x.dim() != 4 or dy.shape[:3] != x.shape[:3] or dy.shape[1] != dy.shape[2]:
        raise ValueError("%s: dy / x must be NHWC [B][hw][hw][cout] / [B][hw][hw][cin_pad]" % who)
    B, hw, _, cout = dy.shape
    cin_pad = x.shape[3]
    _f32_cuda(who, dy, dy=dy, x=x, w_packed=w_packed, bias=bias, mom_w=mom_w, mom_b=mom_b, dx=dx, mask=mask, zeros=zeros)
    if (tuple(w_packed.shape) != (cout, 9, cin_pad) or mom_w.shape != w_packed.shape or tuple(bias.shape) != (cout,)
            or mom_b.shape != bias.shape or (dx is not None and tuple(dx.shape) != (B, hw, hw, cin))
            or (mask is not None and (dx is None or mask.shape != dx.shape))):
        raise ValueError("%s: w_packed / bias / momentum buffers / dx / mask do not match dy and x" % who)
    if zeros is None:
        zeros = torch.zeros(max(512, cin), dtype=torch.float32, device=dy.device)
    if scratch is None:
        sizes, _ = train_conv_backward_scratch(B, hw, cin, cin_pad, cout, dy.device.index)
        scratch = tuple(torch.empty(n, dtype=torch.float32, device=dy.device) for n in sizes)
    slab, wt, bpart = scratch
    _f32_cuda(who, dy, slab=slab, wt=wt, bpart=bpart)
    have = (ctypes.c_size_t * 3)(slab.numel(), wt.numel() if wt is not None else 0, bpart.numel())
    info = ctypes.create_string_buffer(192)
    _ffi.check(_ffi.lib().va_train_conv_backward_layer(
        _ffi.ctx(dy.device.index), int(kernel_opt), B, hw, int(cin), cin_pad, cout, _ffi.ptr(dy), _ffi.ptr(x), _ffi.ptr(w_packed),
        _ffi.ptr(bias), _ffi.ptr(mom_w), _ffi.ptr(mom_b), float(lr), float(momentum), _ffi.ptr(dx), _ffi.ptr(mask), _ffi.ptr(zeros),
        _ffi.ptr(slab), _ffi.ptr(wt), _ffi.ptr(bpart), have, info, len(info), _ffi.stream_ptr(dy.device)))
    return _parse_plan(info.value.decode())


def train_fc_backward_layer(dz, x, w, bias, mom_w, mom_b, lr, momentum, dx, mask=None, scale=1.0):
    """Backward of one Linear layer as the training step does it (``va_train_fc_backward_layer``): dz [B][O], x [B][I],
    w / mom_w [O][I], bias / mom_b [O], dx [B][I], mask [B][I] or None; updates in place; returns the instantiation
    ("k_fc_dx<32>" or "k_fc_dx<64>")."""
    who = "train_fc_backward_layer"
    if dz.dim() != 2 or x.dim() != 2 or dz.shape[0] != x.shape[0]:
        raise ValueError("%s: dz / x must be [B][O] / [B][I]" % who)
    (B, O), I = dz.shape, x.shape[1]
    _f32_cuda(who, dz, dz=dz, x=x, w=w, bias=bias, mom_w=mom_w, mom_b=mom_b, dx=dx, mask=mask)
    if (tuple(w.shape) != (O, I) or mom_w.shape != w.shape or tuple(bias.shape) != (O,) or mom_b.shape != bias.shape
            or dx.shape != x.shape or (mask is not None and mask.shape != x.shape)):
        raise ValueError("%s: w / bias / momentum buffers / dx / mask do not match dz and x" % who)
    info = ctypes.create_string_buffer(64)
    _ffi.check(_ffi.lib().va_train_fc_backward_layer(
        _ffi.ctx(dz.device.index), B, O, I, _ffi.ptr(dz), _ffi.ptr(x), _ffi.ptr(w), _ffi.ptr(bias), _ffi.ptr(mom_w), _ffi.ptr(mom_b),
        float(lr), float(momentum), _ffi.ptr(dx), _ffi.ptr(mask), float(scale), info, len(info), _ffi.stream_ptr(dz.device)))
    return info.value.decode()


def train_conv_backward_layer_grad(dy, x, w_packed, grad_w, grad_b, cin, add, dx=None, mask=None, kernel_opt=1, zeros=None, scratch=None):
    """``train_conv_backward_layer`` in the forms ``train_accumulate`` uses (``va_train_conv_backward_layer_grad``, DESIGN.md
    S29): grad_w ``[cout][9][cin_pad]`` and grad_b ``[cout]`` receive the gradient (``add`` False) or have it added (True);
    w_packed is only read.  Returns the plan that ran."""
    who = "train_conv_backward_layer_grad"
    if dy.dim() != 4 or x.dim() != 4 or dy.shape[:3] != x.shape[:3] or dy.shape[1] != dy.shape[2]:
        raise ValueError("%s: dy / x must be NHWC [B][hw][hw][cout] / [B][hw][hw][cin_pad]" % who)
    B, hw, _, cout = dy.shape
    cin_pad = x.shape[3]
    _f32_cuda(who, dy, dy=dy, x=x, w_packed=w_packed, grad_w=grad_w, grad_b=grad_b, dx=dx, mask=mask, zeros=zeros)
    if (tuple(w_packed.shape) != (cout, 9, cin_pad) or grad_w.shape != w_packed.shape or tuple(grad_b.shape) != (cout,)
            or (dx is not None and tuple(dx.shape) != (B, hw, hw, cin)) or (mask is not None and (dx is None or mask.shape != dx.shape))):
        raise ValueError("%s: w_packed / grad_w / grad_b / dx / mask do not match dy and x" % who)
    if zeros is None:
        zeros = torch.zeros(max(512, cin), dtype=torch.float32, device=dy.device)
    if scratch is None:
        sizes, _ = train_conv_backward_scratch(B, hw, cin, cin_pad, cout, dy.device.index)
        scratch = tuple(torch.empty(n, dtype=torch.float32, device=dy.device) for n in sizes)
    slab, wt, bpart = scratch
    _f32_cuda(who, dy, slab=slab, wt=wt, bpart=bpart)
    have = (ctypes.c_size_t * 3)(slab.numel(), wt.numel() if wt is not None else 0, bpart.numel())
    info = ctypes.create_string_buffer(192)
    _ffi.check(_ffi.lib().va_train_conv_backward_layer_grad(
        _ffi.ctx(dy.device.index), int(kernel_opt), B, hw, int(cin), cin_pad, cout, _ffi.ptr(dy), _ffi.ptr(x), _ffi.ptr(w_packed),
        int(bool(add)), _ffi.ptr(grad_w), _ffi.ptr(grad_b), _ffi.ptr(dx), _ffi.ptr(mask), _ffi.ptr(zeros), _ffi.ptr(slab), _ffi.ptr(wt),
        _ffi.ptr(bpart), have, info, len(info), _ffi.stream_ptr(dy.device)))
    return _parse_plan(info.value.decode())


def train_fc_backward_layer_grad(dz, x, w, grad_w, grad_b, add, dx, mask=None, scale=1.0):
    """``train_fc_backward_layer`` in the forms ``train_accumulate`` uses (``va_train_fc_backward_layer_grad``): grad_w
    ``[O][I]`` and grad_b ``[O]`` receive the gradient (``add`` False) or have it added (True); w is only read."""
    who = "train_fc_backward_layer_grad"
    if dz.dim() != 2 or x.dim() != 2 or dz.shape[0] != x.shape[0]:
        raise ValueError("%s: dz / x must be [B][O] / [B][I]" % who)
    (B, O), I = dz.shape, x.shape[1]
    _f32_cuda(who, dz, dz=dz, x=x, w=w, grad_w=grad_w, grad_b=grad_b, dx=dx, mask=mask)
    if (tuple(w.shape) != (O, I) or grad_w.shape != w.shape or tuple(grad_b.shape) != (O,) or dx.shape != x.shape
            or (mask is not None and mask.shape != x.shape)):
        raise ValueError("%s: w / grad_w / grad_b / dx / mask do not match dz and x" % who)
    info = ctypes.create_string_buffer(64)
    _ffi.check(_ffi.lib().va_train_fc_backward_layer_grad(
        _ffi.ctx(dz.device.index), B, O, I, _ffi.ptr(dz), _ffi.ptr(x), _ffi.ptr(w), int(bool(add)), _ffi.ptr(grad_w), _ffi.ptr(grad_b),
        _ffi.ptr(dx), _ffi.ptr(mask), float(scale), info, len(info), _ffi.stream_ptr(dz.device)))
    return info.value.decode()


def train_pool_layer(y, p, dp=None, dy=None):
    """``va_train_pool_layer``: p = 2x2/2 max-pool of y (NHWC float32) and, with dp and dy, the step's max-pool backward
    (first maximum in row-major order, nothing where the pooled value is <= 0)."""
    who = "train_pool_layer"
    if y.dim() != 4 or y.shape[1] != y.shape[2]:
        raise ValueError("%s: y must be NHWC [B][hw][hw][c]" % who)
    B, hw, _, c = y.shape
    _f32_cuda(who, y, y=y, p=p, dp=dp, dy=dy)
    if tuple(p.shape) != (B, hw // 2, hw // 2, c) or (dp is not None and dp.shape != p.shape) or (dy is not None and dy.shape != y.shape):
        raise ValueError("%s: p / dp / dy do not match y" % who)
    _ffi.check(_ffi.lib().va_train_pool_layer(_ffi.ctx(y.device.index), B, hw, c, _ffi.ptr(y), _ffi.ptr(p), _ffi.ptr(dp), _ffi.ptr(dy),
                                              _ffi.stream_ptr(y.device)))


def train_loss(logits, labels, dlogits, out, k=0):
    """``va_train_loss``: logits [n][c] (k = 0) or [n][k][c]; labels int64 [n] on the device; dlogits like logits;
    out float32 [2] = mean cross-entropy (of the snippet consensus when k >= 1), hits."""
    who = "train_loss"
    _f32_cuda(who, logits, logits=logits, dlogits=dlogits, out=out)
    n, c = logits.shape[0], logits.shape[-1]
    if (tuple(logits.shape) != ((n, c) if k == 0 else (n, k, c)) or dlogits.shape != logits.shape or out.numel() < 2
            or labels.dtype != torch.int64 or tuple(labels.shape) != (n,) or labels.device != logits.device or not labels.is_contiguous()):
        raise ValueError("%s: logits / labels / dlogits / out do not match" % who)
    _ffi.check(_ffi.lib().va_train_loss(_ffi.ctx(logits.device.index), _ffi.ptr(logits), _ffi.ptr(labels), n, int(k), c, _ffi.ptr(dlogits),
                                        _ffi.ptr(out), _ffi.stream_ptr(logits.device)))


def train_loss_multitask(logits, labels, tasks, heads, dlogits, out, k=0):
    """``va_train_loss_multitask``: logits [n][c] (k = 0) or [n][k][c] with c = sum(heads); labels int64 [n],
    local to the video's head, and tasks int32 [n], both on the device; dlogits like logits; out float32 [2 + 2 len(heads)] =
    loss, hits, the loss of every head, the hits of every head."""
    who = "train_loss_multitask"
    _f32_cuda(who, logits, logits=logits, dlogits=dlogits, out=out)
    n, c = logits.shape[0], logits.shape[-1]
    check_heads(heads, c, who)
    heads = [int(h) for h in heads]
    if (tuple(logits.shape) != ((n, c) if k == 0 else (n, k, c)) or dlogits.shape != logits.shape or out.numel() < 2 + 2 * len(heads)
            or labels.dtype != torch.int64 or tuple(labels.shape) != (n,) or labels.device != logits.device or not labels.is_contiguous()
            or tasks.dtype != torch.int32 or tuple(tasks.shape) != (n,) or tasks.device != logits.device or not tasks.is_contiguous()):
        raise ValueError("%s: logits / labels / tasks / dlogits / out do not match" % who)
    _ffi.check(_ffi.lib().va_train_loss_multitask(_ffi.ctx(logits.device.index), _ffi.ptr(logits), _ffi.ptr(labels), _ffi.ptr(tasks), n, int(k),
                                                  len(heads), (ctypes.c_int * len(heads))(*heads), _ffi.ptr(dlogits), _ffi.ptr(out),
                                                  _ffi.stream_ptr(logits.device)))


def train_dropout(x, seed, layer, p=0.5):
    """``va_train_dropout`` / ``va_train_dropout_p``: the step's Dropout(p) of classifier layer ``layer`` (0..2) in place on
    float32 x.  The default ratio goes through the entry point that has no ratio argument; both give the same bits."""
    _f32_cuda("train_dropout", x, x=x)
    if p == 0.5:
        _ffi.check(_ffi.lib().va_train_dropout(_ffi.ctx(x.device.index), _ffi.ptr(x), x.numel(), int(seed), int(layer), _ffi.stream_ptr(x.device)))
        return
    p = _solver_ratio("train_dropout", "p", p)
    _ffi.check(_ffi.lib().va_train_dropout_p(_ffi.ctx(x.device.index), _ffi.ptr(x), x.numel(), int(seed), int(layer), p,
                                             _ffi.stream_ptr(x.device)))


# ---- the solver, host side: no device is touched here ----

def _f32(v):
    """The float32 nearest to v, as a Python float (what crosses the C ABI)."""
    return ctypes.c_float(v).value


def _solver_number(who, name, v):
    import math
    import numbers
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise ValueError("%s: %s must be a number, got %r" % (who, name, v))
    f = _f32(float(v)) if math.isfinite(v) else float(v)
    if not math.isfinite(f) or f < 0.0:
        raise ValueError("%s: %s must be finite (as a float32) and >= 0, got %r" % (who, name, v))
    return f


def _solver_ratio(who, name, v):
    import math
    import numbers
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or math.isnan(v):
        raise ValueError("%s: %s must be a number in [0, 1), got %r" % (who, name, v))
    f = _f32(float(v)) if math.isfinite(v) else float(v)
    if not 0.0 <= f < 1.0:
        raise ValueError("%s: %s must lie in [0, 1) as a float32, got %r" % (who, name, v))
    return f


def dropout_threshold(p):
    """T of Dropout(p): an element is kept iff the top 24 bits of its hash reach ``T = ceil(float32(p) * 2**24)``, that is
    iff ``synth.hash_uniform(...) >= float32(p)``."""
    import math
    return int(math.ceil(_solver_ratio("dropout_threshold", "p", p) * 16777216.0))


def dropout_scale(p):
    """s of Dropout(p): ``float32(1) / (float32(1) - float32(p))``, the factor of a kept element."""
    p = _solver_ratio("dropout_scale", "p", p)
    return _f32(1.0 / _f32(1.0 - p))


class Solver(object):
    """The solver state of a ``Vgg16Stream`` (``va_solver``): ``weight_decay`` (torch.optim.SGD's L2
    coefficient), ``bias_lr_mult`` / ``bias_decay_mult`` (a bias uses ``lr * bias_lr_mult`` and ``weight_decay *
    bias_decay_mult``; Caffe's VGG and TSN solvers: 2 and 0), ``dropout``: the ratio of the classifier's three Dropout layers,
    one number or three, each in [0, 1), and ``freeze``: the first n of the 17 layers (conv 0..12, fc 0..3) take no gradient
    and no update, n in 0..16.  Checked here (ValueError); every number is held as the float32 the library receives."""

    def __init__(self, weight_decay=0.0, bias_lr_mult=1.0, bias_decay_mult=1.0, dropout=0.5, freeze=0):
        import numbers
        who = "Solver"
        self.weight_decay = _solver_number(who, "weight_decay", weight_decay)
        self.bias_lr_mult = _solver_number(who, "bias_lr_mult", bias_lr_mult)
        self.bias_decay_mult = _solver_number(who, "bias_decay_mult", bias_decay_mult)
        if isinstance(dropout, numbers.Real) and not isinstance(dropout, bool):
            dropout = (dropout,) * 3
        try:
            dropout = tuple(dropout)
        except TypeError:
            raise ValueError("%s: dropout must be a number or three numbers, got %r" % (who, dropout))
        if len(dropout) != 3:
            raise ValueError("%s: dropout must be a number or three numbers, got %r" % (who, dropout))
        self.dropout = tuple(_solver_ratio(who, "dropout[%d]" % i, v) for i, v in enumerate(dropout))
        if isinstance(freeze, bool) or not isinstance(freeze, numbers.Integral) or not 0 <= freeze <= 16:
            raise ValueError("%s: freeze must be an integer in 0..16, got %r" % (who, freeze))
        self.freeze = int(freeze)

    def _key(self):
        return (self.weight_decay, self.bias_lr_mult, self.bias_decay_mult, self.dropout, self.freeze)

    def __eq__(self, other):
        return isinstance(other, Solver) and self._key() == other._key()

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "Solver(weight_decay=%r, bias_lr_mult=%r, bias_decay_mult=%r, dropout=%r, freeze=%r)" % self._key()

    def to_struct(self):
        s = _ffi.SolverParams()
        s.weight_decay, s.bias_lr_mult, s.bias_decay_mult = self.weight_decay, self.bias_lr_mult, self.bias_decay_mult
        for i in range(3):
            s.dropout[i] = self.dropout[i]
        s.frozen_layers = self.freeze
        return s

    @classmethod
    def from_struct(cls, s):
        return cls(s.weight_decay, s.bias_lr_mult, s.bias_decay_mult, tuple(s.dropout), s.frozen_layers)


def check_solver(solver, who):
    """``solver`` argument of the training surfaces: None or a ``Solver``."""
    if solver is not None and not isinstance(solver, Solver):
        raise ValueError("%s: solver must be None or a vgg.Solver, got %r" % (who, solver))
    return solver


def _ffi_conv_cout(i):
    return (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)[i]


def _check_labels(labels, n_classes, who):
    """``nn.CrossEntropyLoss`` (Sheet03/spatialModel.py:114,219) refuses a target outside [0, C) ("Target 101 is out
    of bounds"); the datasets return the list files' raw 1-based labels, so the full UCF-101 list
    with ``nActionClasses = 101`` does trip this.  Labels still on the host (what a DataLoader hands over) are
    checked here without touching the GPU; labels already on the device are not copied back -- for those the
    kernels read nothing out of bounds and return a NaN loss."""
    if isinstance(labels, torch.Tensor) and not labels.is_cuda and labels.numel() > 0:
        lo, hi = int(labels.min()), int(labels.max())
        if lo < 0 or hi >= n_classes:
            raise ValueError("%s: Target %d is out of bounds for %d classes" % (who, hi if hi >= n_classes else lo, n_classes))


MAX_HEADS = 8  # VA_MAX_HEADS of the library


# ---- gradient accumulation, host side: no device is touched here ----

def check_scales(scales, n, who):
    """``scales`` of ``train_accumulate`` -> a list of n finite floats (None: ones; a number: that number n times)."""
    import math
    import numbers
    if scales is None:
        return [1.0] * n
    if isinstance(scales, numbers.Real) and not isinstance(scales, bool):
        scales = [scales] * n
    try:
        out = [float(v) for v in scales]
    except (TypeError, ValueError):
        raise ValueError("%s: scales must be None, a number or %d numbers, got %r" % (who, n, scales))
    if len(out) != n or not all(math.isfinite(v) for v in out):
        raise ValueError("%s: scales must be %d finite numbers, got %r" % (who, n, scales))
    return out


def check_clip_norm(clip_norm, who):
    """None -> 0.0 (no clipping); a finite positive number -> float; ValueError otherwise."""
    import math
    import numbers
    if clip_norm is None:
        return 0.0
    if isinstance(clip_norm, bool) or not isinstance(clip_norm, numbers.Real) or not math.isfinite(clip_norm) or clip_norm <= 0:
        raise ValueError("%s: clip_norm must be None or a finite positive number, got %r" % (who, clip_norm))
    return float(clip_norm)


def micro_slices(n, m):
    """The micro-batches of n videos, at most m each, in order: [(lo, hi), ...]; ``ceil(n/m)`` of them, the last one ragged."""
    n, m = int(n), int(m)
    if n < 1 or m < 1:
        raise ValueError("micro_slices: need n >= 1 and m >= 1, got n=%d m=%d" % (n, m))
    return [(lo, min(lo + m, n)) for lo in range(0, n, m)]


def micro_scales(slices, n_total=None, tasks=None, n_heads=0, head_totals=None):
    """The scales of the micro-batches ``slices``: what makes the sum of their mean losses the full batch's mean.  Without
    heads: ``[(hi - lo) / n_total]`` per slice (n_total None: the videos of the slices).  With ``tasks`` (one head index per
    video, on the host) and ``n_heads``: per slice one scale per head, the head's videos in the slice over its videos in the
    batch (``head_totals``; None: counted from tasks).  A head absent from the slice, or from the whole batch, gets 0: its
    columns' gradient is exactly zero anyway.  Data-parallel steps pass the totals over all ranks."""
    if tasks is None:
        total = sum(hi - lo for lo, hi in slices) if n_total is None else int(n_total)
        return [[float(hi - lo) / float(total)] for lo, hi in slices]
    tasks = [int(t) for t in tasks]
    if head_totals is None:
        head_totals = [sum(1 for t in tasks if t == h) for h in range(n_heads)]
    out = []
    for lo, hi in slices:
        cnt = [sum(1 for t in tasks[lo:hi] if t == h) for h in range(n_heads)]
        out.append([float(c) / float(tot) if tot > 0 else 0.0 for c, tot in zip(cnt, head_totals)])
    return out


def combine_micro_stats(stats, scales, n_heads=0):
    """The ``stats`` of a step of several micro-batches from theirs, on their device in float32: without heads
    (loss, hits) = (sum_j scale_j loss_j, sum_j hits_j), added in micro-batch order from 0; with heads every head's loss is
    weighted by that head's scale, the total loss is the heads' sum in head order, hits add up."""
    dev = stats[0].device
    if n_heads == 0:
        w = torch.tensor([[s[0], 1.0] for s in scales], dtype=torch.float32, device=dev)
        out = torch.zeros(2, dtype=torch.float32, device=dev)
        for j, st in enumerate(stats):
            out = out + w[j] * st
        return out
    H = n_heads
    w = torch.tensor([list(s) + [1.0] * H for s in scales], dtype=torch.float32, device=dev)
    per = torch.zeros(2 * H, dtype=torch.float32, device=dev)
    for j, st in enumerate(stats):
        per = per + w[j] * st[2:]
    loss = torch.zeros((), dtype=torch.float32, device=dev)
    for h in range(H):
        loss = loss + per[h]
    return torch.cat([torch.stack([loss, per[H:].sum()]), per])


def check_heads(heads, n_classes, who):
    """The heads of a multi-task model: ``heads`` = 1 to 8 positive integers, the class counts of the datasets,
    whose sum is ``n_classes``, the outputs of the shared last layer (``None``: any sum).  -> the tuple of their offsets:
    head t owns the logit columns ``[off[t], off[t] + heads[t])``.  ValueError otherwise."""
    import numbers
    try:
        hs = list(heads)
    except TypeError:
        raise ValueError("%s: heads must be a sequence of 1..%d class counts, got %r" % (who, MAX_HEADS, heads))
    if not 1 <= len(hs) <= MAX_HEADS:
        raise ValueError("%s: 1..%d heads, got %d" % (who, MAX_HEADS, len(hs)))
    for h in hs:
        if isinstance(h, bool) or not isinstance(h, numbers.Integral) or h < 1:
            raise ValueError("%s: every head needs a positive integer class count, got %r" % (who, h))
    if n_classes is not None and sum(int(h) for h in hs) != int(n_classes):
        raise ValueError("%s: the heads %s hold %d classes, the last layer %d" % (who, tuple(hs), sum(int(h) for h in hs), n_classes))
    offs, o = [], 0
    for h in hs:
        offs.append(o)
        o += int(h)
    return tuple(offs)


def check_task(task, heads, who):
    """-> ``task`` as an int in ``[0, len(heads))``; ValueError otherwise."""
    import numbers
    if isinstance(task, bool) or not isinstance(task, numbers.Integral) or not 0 <= task < len(heads):
        raise ValueError("%s: task must be the index of one of the %d heads, got %r" % (who, len(heads), task))
    return int(task)


def head_logits(t, heads, task):
    """The class scores of head ``task``: the columns ``[o_task, o_task + heads[task])`` of the last dimension of a logits
    tensor of ``sum(heads)`` columns (``submit`` / ``run_batch`` and ``Vgg16Stream.forward`` return all heads side by
    side), as a contiguous tensor."""
    if not isinstance(t, torch.Tensor) or t.dim() < 1:
        raise ValueError("head_logits: a logits tensor [..., sum(heads)] is needed")
    offs = check_heads(heads, int(t.shape[-1]), "head_logits")
    task = check_task(task, list(heads), "head_logits")
    return t[..., offs[task]:offs[task] + int(list(heads)[task])].contiguous()


def check_tasks(labels, tasks, heads, n, who):
    """The host-side checks of a multi-task batch -> (labels, tasks) as tensors ``[n]`` (lists become CPU tensors).  What is
    still on the host is checked without touching the GPU: every task in ``[0, len(heads))`` and, head by head,
    ``_check_labels`` of that head's videos against its class count.  Tensors already on the device are not copied back:
    for those the kernel reads nothing out of bounds and returns a NaN loss."""
    def as_tensor(v, name, dtype):
        if isinstance(v, torch.Tensor):
            if v.dtype not in (torch.int32, torch.int64):
                raise ValueError("%s: %s must be an integer tensor, got %s" % (who, name, v.dtype))
            return v
        try:
            return torch.tensor([int(e) for e in v], dtype=dtype)
        except (TypeError, ValueError):
            raise ValueError("%s: %s must be a tensor or a list of %d integers" % (who, name, n))
    labels = as_tensor(labels, "labels", torch.int64)
    tasks = as_tensor(tasks, "tasks", torch.int32)
    if labels.dim() != 1 or labels.shape[0] != n:
        raise ValueError("%s: labels must be [%d], one per video, got %s" % (who, n, tuple(labels.shape)))
    if tasks.dim() != 1 or tasks.shape[0] != n:
        raise ValueError("%s: tasks must be [%d], one head per video, got %s" % (who, n, tuple(tasks.shape)))
    heads = [int(h) for h in heads]
    if not tasks.is_cuda and n > 0:
        lo, hi = int(tasks.min()), int(tasks.max())
        if lo < 0 or hi >= len(heads):
            raise ValueError("%s: task %d is not one of the %d heads" % (who, hi if hi >= len(heads) else lo, len(heads)))
        if not labels.is_cuda:
            for t, c in enumerate(heads):
                _check_labels(labels[tasks == t], c, "%s (head %d)" % (who, t))
    return labels, tasks


def view_mean(x):
    """x: CUDA float32 ``[B,V,...]`` -> ``[B,...]``, the mean over the V views (``va_view_mean``): summed in view order,
    ``((x[:,0] + x[:,1]) + ...) + x[:,V-1]``, then divided by V once."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() < 2:
        raise ValueError("view_mean: x must be a CUDA float32 tensor [B,V,...]")
    x = x.contiguous()
    B, V = int(x.shape[0]), int(x.shape[1])
    d = x.numel() // max(1, B * V)
    out = torch.empty((B,) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    _ffi.check(_ffi.lib().va_view_mean(_ffi.ctx(x.device.index), _ffi.ptr(x), B, V, d, _ffi.ptr(out),
                                       _ffi.stream_ptr(x.device)))
    return out


def validate_batch(logits, labels):
    """(mean cross-entropy, number correct) of one batch on the device
    (Sheet03/spatialModel.py:219-221); returns a CUDA float32 tensor [2] without synchronising."""
    if not logits.is_cuda or logits.dtype != torch.float32 or logits.dim() != 2:
        raise ValueError("validate_batch: logits must be CUDA float32 [B,C]")
    _check_labels(labels, logits.shape[1], "validate_batch")
    labels = labels.to(device=logits.device, dtype=torch.int64).contiguous()
    if labels.dim() != 1 or labels.shape[0] != logits.shape[0]:
        raise ValueError("validate_batch: labels must be [B]")
    logits = logits.contiguous()
    out = torch.empty(2, dtype=torch.float32, device=logits.device)
    _ffi.check(_ffi.lib().va_validate_batch(_ffi.ctx(logits.device.index), _ffi.ptr(logits), _ffi.ptr(labels),
                                            logits.shape[0], logits.shape[1], _ffi.ptr(out), _ffi.stream_ptr(logits.device)))
    return out
