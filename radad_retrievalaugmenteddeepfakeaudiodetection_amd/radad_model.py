"""RADADModel / DetectionModel -- inference forward of radad_model.py:9-41 and detection_model.py:9-125 on the GPU.

Module tree and parameter names equal the reference's (`projection_layer.*`, `fuse.*`, `detection_model.model.<i>.*`
with the same nn.Sequential indices), so `load_state_dict` of a reference checkpoint works unchanged.  forward()
runs csrc/proj.hip: the projection (one pass over the neighbour tensor), then `radad_fuse_head_forward` --
fuse Linear over [tpp ; proj] without building the concatenation, and the detection MLP with BatchNorm in its
eval form (running statistics as scale/shift).  Training is opt-in (`config.projection_train_hip = True`): a training-mode
forward then runs the projection's HIP forward + backward (csrc/proj_train.inc) and the fuse Linear and the detection MLP as the
plain torch modules they are (BatchNorm updates its running statistics as in the reference).  With `config.head_train_hip = True`
as well, fuse and the detection MLP train in HIP too (`_FuseHeadTrainFn`, csrc/head_train.inc: batch statistics, running statistics
updated in place, dropout by masks torch draws), so the whole step from the neighbour tensor to the logits and back is HIP; that key
alone makes `fuse_and_detect` train while forward() still raises from the projection.  With the defaults a training-mode forward
raises, and training stays in the reference.
"""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from .projection import ProjectionLayer


class HeadTrainSpec:
    """What _FuseHeadTrainFn needs beside tensors that take gradients.  Per hidden layer i (len(bn) = number of hidden layers):
    bn[i]: the layer has a BatchNorm1d; eps[i], factor[i]: its eps and running-statistics update factor; running[i]: (mean, var)
    float32 buffers updated in place by the forward, or None; masks[i]: [B, d_i] float32 tensor of 0 / 1, or None."""

    def __init__(self, bn, eps=None, factor=None, running=None, masks=None, inv_keep=1.0):
        n = len(bn)
        self.bn = [bool(b) for b in bn]
        self.eps = [1e-5] * n if eps is None else [float(e) for e in eps]
        self.factor = [0.1] * n if factor is None else [float(f) for f in factor]
        self.running = [None] * n if running is None else list(running)
        self.masks = [None] * n if masks is None else list(masks)
        self.inv_keep = float(inv_keep)
        if not (len(self.eps) == len(self.factor) == len(self.running) == len(self.masks) == n):
            raise ValueError("HeadTrainSpec: one entry per hidden layer in every list")


def _check_head_train_inputs(tpp, proj, spec, params):
    """TypeError / ValueError unless everything the kernels index through raw pointers is a float32 tensor on tpp's ROCm device
    with the shape they assume.  Returns the layer widths [P, d_1, ..., d_out]."""
    _lib.require_cuda(tpp, "tpp_vecs")
    if tpp.dim() != 2 or proj.dim() != 2 or proj.shape[0] != tpp.shape[0]:
        raise ValueError(f"expected tpp [B, D] and proj [B, P], got {tuple(tpp.shape)} and {tuple(proj.shape)}")
    (B, D), P = tpp.shape, proj.shape[1]
    n_hidden = len(spec.bn)
    if len(params) != 2 + 2 * (n_hidden + 1) + 2 * sum(spec.bn):
        raise ValueError(f"expected fuse weight and bias, weight and bias per layer and gamma, beta per BatchNorm layer; got "
                         f"{len(params)} tensors for {n_hidden} hidden layers")
    if n_hidden + 1 > _lib.HEAD_MAX_LAYERS:
        raise ValueError(f"at most {_lib.HEAD_MAX_LAYERS} Linear layers in the detection head")
    named = [("tpp_vecs", tpp, (B, D)), ("proj", proj, (B, P)), ("fuse.weight", params[0], (P, D + P)), ("fuse.bias", params[1], (P,))]
    dims, i = [P], 2
    for l in range(n_hidden + 1):
        if not isinstance(params[i], torch.Tensor) or params[i].dim() != 2:
            raise ValueError(f"layer {l}: the weight must be a matrix")
        d = params[i].shape[0]
        named += [(f"layer {l} weight", params[i], (d, dims[-1])), (f"layer {l} bias", params[i + 1], (d,))]
        i += 2
        if l < n_hidden:
            if spec.bn[l]:
                named += [(f"layer {l} BatchNorm weight", params[i], (d,)), (f"layer {l} BatchNorm bias", params[i + 1], (d,))]
                i += 2
                if spec.running[l] is not None:
                    named += [(f"layer {l} running_mean", spec.running[l][0], (d,)), (f"layer {l} running_var", spec.running[l][1], (d,))]
            if spec.masks[l] is not None:
                named.append((f"layer {l} dropout mask", spec.masks[l], (B, d)))
        dims.append(d)
    for name, t, shape in named:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"{name} must be a float32 tensor (cast with .float(); RADADModel.fuse_and_detect does), got "
                            f"{getattr(t, 'dtype', type(t))}")
        if t.device != tpp.device:
            raise ValueError(f"{name} is on {t.device}, tpp_vecs on {tpp.device}")
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}")
    for l in range(n_hidden):
        if spec.running[l] is not None and not all(r.is_contiguous() for r in spec.running[l]):
            raise ValueError(f"layer {l}: running statistics must be contiguous (they are updated in place)")
    if B == 1 and any(spec.bn):
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {torch.Size([B, dims[1]])}")
    return dims


def _head_structs(spec, params, dims, saved, grads=None):
    """(HeadTrainWeights, HeadSaved, HeadGrads | None, masks array) of device pointers for contiguous float32 tensors."""
    n_hidden = len(spec.bn)
    w, sv, masks = _lib.HeadTrainWeights(), _lib.HeadSaved(), _lib.HeadMasks()
    gr = _lib.HeadGrads() if grads is not None else None
    ptr = lambda t: None if t is None else t.data_ptr()
    w.wf, w.bf, w.n_layers = ptr(params[0]), ptr(params[1]), n_hidden + 1
    for j, d in enumerate(dims):
        w.dims[j] = d
    sv.fused = ptr(saved[0])
    if gr is not None:
        gr.dwf, gr.dbf = ptr(grads[0]), ptr(grads[1])
    i = 2
    for l in range(n_hidden + 1):
        w.lw[l], w.lb[l] = ptr(params[i]), ptr(params[i + 1])
        if gr is not None:
            gr.dlw[l], gr.dlb[l] = ptr(grads[i]), ptr(grads[i + 1])
        i += 2
        if l < n_hidden:
            sv.xh[l], sv.rstd[l], sv.act[l] = (ptr(t) for t in saved[1 + 3 * l:4 + 3 * l])
            masks[l] = ptr(spec.masks[l])
            if spec.bn[l]:
                w.bn_gamma[l], w.bn_beta[l] = ptr(params[i]), ptr(params[i + 1])
                if gr is not None:
                    gr.dgamma[l], gr.dbeta[l] = ptr(grads[i]), ptr(grads[i + 1])
                i += 2
                w.bn_eps[l], w.bn_factor[l] = spec.eps[l], spec.factor[l]
                if spec.running[l] is not None:
                    w.bn_running_mean[l], w.bn_running_var[l] = ptr(spec.running[l][0]), ptr(spec.running[l][1])
    return w, sv, gr, masks


def _head_train_workspace(lib, t, B, D, dims):
    need = lib.radad_fuse_head_train_workspace_bytes(B, D, dims[0], len(dims) - 1, (C.c_int32 * len(dims))(*dims))
    if need < 0:
        raise ValueError(f"head training: shape B={B} D={D} widths={dims} is outside the kernels' limits")
    return torch.empty(max(int(need), 1), dtype=torch.uint8, device=t.device)


class _FuseHeadTrainFn(torch.autograd.Function):
    """radad_model.py:39-40 in training mode with a hand-written backward (csrc/head_train.inc): the fuse Linear over [tpp ; proj]
    without the concatenation, then per hidden layer Linear -> BatchNorm1d (batch statistics; the running statistics in
    spec.running are updated in place) -> ReLU -> dropout by the caller's mask, then the output Linear.  fp32: under autocast
    the inputs are cast to fp32 and the logits are fp32.
    apply(tpp [B,D], proj [B,P], spec: HeadTrainSpec, fuse.weight, fuse.bias, then per layer weight, bias and -- for a hidden layer
    with BatchNorm -- gamma, beta) -> (logits [B, d_out], fused [B,P] without a gradient).  Every tensor must be float32 (TypeError otherwise).  A parameter that
    needs no gradient is not computed (NULL in radad_head_grads); dtpp is computed only when tpp requires a gradient."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, tpp, proj, spec, *params):
        lib = _lib.load()
        dims = _check_head_train_inputs(tpp, proj, spec, params)
        tpp, proj = tpp.contiguous(), proj.contiguous()
        params = tuple(p.contiguous() for p in params)
        spec.masks = [None if m is None else m.contiguous() for m in spec.masks]
        B, D = tpp.shape
        new = lambda *shape: torch.empty(shape, device=tpp.device, dtype=torch.float32)
        saved = [new(B, dims[0])]
        for l, d in enumerate(dims[1:-1]):
            saved += [new(B, d), new(d) if spec.bn[l] else None, new(B, d)]          # xh, rstd, act
        logits = new(B, dims[-1])
        ws = _head_train_workspace(lib, tpp, B, D, dims)
        w, sv, _, masks = _head_structs(spec, params, dims, saved)
        with torch.cuda.device(tpp.device):
            _lib.check(lib.radad_fuse_head_train_forward(C.byref(w), tpp.data_ptr(), proj.data_ptr(), masks, spec.inv_keep, B, D,
                                                         dims[0], C.byref(sv), logits.data_ptr(), ws.data_ptr(), int(ws.numel()),
                                                         tpp.device.index, _lib.stream_ptr(tpp.device)),
                       "radad_fuse_head_train_forward")
        ctx.save_for_backward(tpp, proj, *params, *[t for t in saved if t is not None],
                              *[m for m in spec.masks if m is not None])
        ctx.spec, ctx.dims, ctx.n_params = spec, dims, len(params)
        ctx.mark_non_differentiable(saved[0])
        return logits, saved[0]

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_logits, _grad_fused):
        lib = _lib.load()
        spec, dims = ctx.spec, ctx.dims
        tensors = list(ctx.saved_tensors)
        tpp, proj, params = tensors[0], tensors[1], tensors[2:2 + ctx.n_params]
        rest = tensors[2 + ctx.n_params:]
        saved = [rest.pop(0)]
        for l in range(len(spec.bn)):
            xh = rest.pop(0)
            rstd = rest.pop(0) if spec.bn[l] else None
            saved += [xh, rstd, rest.pop(0)]
        bspec = HeadTrainSpec(spec.bn, spec.eps, spec.factor, None, [None if m is None else rest.pop(0) for m in spec.masks],
                              spec.inv_keep)
        g = grad_logits.contiguous().float()            # logits.sum().backward() hands over a stride-0 expand
        B, D = tpp.shape
        need = ctx.needs_input_grad
        grads = [torch.empty(p.shape, device=tpp.device, dtype=torch.float32) if need[3 + i] else None for i, p in enumerate(params)]
        dtpp = torch.empty(tpp.shape, device=tpp.device, dtype=torch.float32) if need[0] else None
        dproj = torch.empty(proj.shape, device=tpp.device, dtype=torch.float32) if need[1] else None
        ws = _head_train_workspace(lib, tpp, B, D, dims)
        w, sv, gr, masks = _head_structs(bspec, params, dims, saved, grads)
        ptr = lambda t: None if t is None else t.data_ptr()
        with torch.cuda.device(tpp.device):
            _lib.check(lib.radad_fuse_head_backward(C.byref(w), tpp.data_ptr(), proj.data_ptr(), masks, spec.inv_keep, C.byref(sv),
                                                    g.data_ptr(), B, D, dims[0], C.byref(gr), ptr(dtpp), ptr(dproj), ws.data_ptr(),
                                                    int(ws.numel()), tpp.device.index, _lib.stream_ptr(tpp.device)),
                       "radad_fuse_head_backward")
        return (dtpp, dproj, None) + tuple(grads)


class DetectionModel(nn.Module):
    """detection_model.py:9-72: [input_dim] + detection_hidden_dims + [1]; Linear (+ BatchNorm1d | LayerNorm) + ReLU
    + Dropout per hidden layer, Linear alone for the output.  Holds parameters only; RADADModel runs it."""

    def __init__(self, config, input_dim: int):
        super().__init__()
        self.config = config
        self.device = torch.device(getattr(config, "device", "cuda"))
        self.use_batch_norm = bool(getattr(config, "use_batch_norm", True))
        self.use_layer_norm = bool(getattr(config, "use_layer_norm", False))
        self.layers_dims = [int(input_dim)] + [int(d) for d in config.detection_hidden_dims] + [1]
        self.num_layers = len(self.layers_dims) - 1
        if self.num_layers > _lib.HEAD_MAX_LAYERS:
            raise ValueError(f"at most {_lib.HEAD_MAX_LAYERS} Linear layers in the detection head")
        if self.use_layer_norm and not self.use_batch_norm:
            raise NotImplementedError("detection head with LayerNorm: only the BatchNorm (default) and plain variants "
                                      "have a HIP forward")
        layers = []
        for i in range(self.num_layers):                                       # detection_model.py:45-70
            layers.append(nn.Linear(self.layers_dims[i], self.layers_dims[i + 1]))
            if i < self.num_layers - 1:
                if self.use_batch_norm:
                    layers.append(nn.BatchNorm1d(self.layers_dims[i + 1]))
                layers.append(nn.ReLU(inplace=True))
                if float(getattr(config, "detection_dropout", 0.1)) > 0:
                    layers.append(nn.Dropout(float(getattr(config, "detection_dropout", 0.1))))
        self.model = nn.Sequential(*layers)
        for m in self.modules():                                               # :93-105
            if isinstance(m, nn.Linear):
                nn.init.kaiming_uniform_(m.weight, nonlinearity="relu")
                nn.init.zeros_(m.bias)
        self.to(self.device)

    def head_layers(self):
        """[(Linear, BatchNorm1d | None)] in forward order."""
        out, mods = [], list(self.model)
        for i, m in enumerate(mods):
            if isinstance(m, nn.Linear):
                bn = mods[i + 1] if i + 1 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm1d) else None
                out.append((m, bn))
        return out


class RADADModel(nn.Module):
    """radad_model.py:9-41.  forward(neighbor_vecs [B,K,D], tpp_vecs [B,D]) -> logits [B]."""

    def __init__(self, config, tpp_output_dim: int):
        super().__init__()
        self.config = config
        self.device = torch.device(getattr(config, "device", "cuda"))
        self.tpp_output_dim = int(tpp_output_dim)
        self.projection_layer = ProjectionLayer(config, tpp_output_dim)        # :23
        p = int(config.projection_output_dim)
        self.fuse = nn.Linear(self.tpp_output_dim + p, p)                      # :24-26
        self.detection_model = DetectionModel(config, p)                       # :27
        self.to(self.device)
        self._ws = None

    def _training_path(self) -> bool:
        return self.training and torch.is_grad_enabled() and bool(getattr(self.config, "projection_train_hip", False))

    def _check_eval(self, *tensors):
        if self.training and torch.is_grad_enabled():
            raise RuntimeError("RADADModel here is inference-only (HIP forward); call .eval() / torch.no_grad(), "
                               "or train with the reference module and load its state_dict")
        for t in tensors:
            _lib.require_cuda(t, "input")

    def fuse_and_detect(self, tpp_vecs: torch.Tensor, proj: torch.Tensor, return_fused: bool = False):
        """radad_model.py:39-40 given the projection output."""
        if self.training and torch.is_grad_enabled() and bool(getattr(self.config, "head_train_hip", False)):
            logits, fused = self._head_train_forward(tpp_vecs, proj)
            return (logits, fused) if return_fused else logits
        if self._training_path():      # torch modules under autograd: fuse Linear over the concatenation, then the MLP
            fused = self.fuse(torch.cat([tpp_vecs, proj], dim=1))
            logits = self.detection_model.model(fused).squeeze(-1)             # detection_model.py:125
            return (logits, fused) if return_fused else logits
        self._check_eval(tpp_vecs, proj)
        t = tpp_vecs.detach().contiguous().float()
        pr = proj.detach().contiguous().float()
        B, D = t.shape
        P = pr.shape[1]
        if D != self.tpp_output_dim or pr.shape[0] != B or P != self.fuse.out_features:
            raise ValueError(f"expected tpp [B,{self.tpp_output_dim}] and proj [B,{self.fuse.out_features}], got "
                             f"{tuple(t.shape)} and {tuple(pr.shape)}")
        lib = _lib.load()
        keep = []

        def ptr(x):
            x = x.detach().contiguous().float()
            keep.append(x)
            return x.data_ptr()
        w = _lib.HeadWeights()
        w.wf, w.bf = ptr(self.fuse.weight), ptr(self.fuse.bias)
        layers = self.detection_model.head_layers()
        w.n_layers = len(layers)
        w.dims[0] = P
        for i, (lin, bn) in enumerate(layers):
            w.dims[i + 1] = lin.out_features
            w.lw[i], w.lb[i] = ptr(lin.weight), ptr(lin.bias)
            if bn is not None:      # eval BatchNorm1d: (x - mean) / sqrt(var + eps) * gamma + beta
                scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.float() + bn.eps)
                shift = bn.bias.detach().float() - bn.running_mean.float() * scale
                w.bn_scale[i], w.bn_shift[i] = ptr(scale), ptr(shift)
        n_out = layers[-1][0].out_features if layers else P
        logits = torch.empty((B, n_out), device=t.device, dtype=torch.float32)
        fused = torch.empty((B, P), device=t.device, dtype=torch.float32) if (return_fused or not layers) else None
        need = lib.radad_fuse_head_workspace_bytes(B, D, P)
        if self._ws is None or self._ws.numel() < need or self._ws.device != t.device:
            self._ws = torch.empty(int(need), dtype=torch.uint8, device=t.device)
        with torch.cuda.device(t.device):
            _lib.check(lib.radad_fuse_head_forward(C.byref(w), t.data_ptr(), pr.data_ptr(), B, D, P,
                                                   fused.data_ptr() if fused is not None else None, logits.data_ptr(),
                                                   self._ws.data_ptr(), int(self._ws.numel()), t.device.index,
                                                   _lib.stream_ptr(t.device)), "radad_fuse_head_forward")
        logits = logits.squeeze(-1)                                            # detection_model.py:125
        return (logits, fused) if return_fused else logits

    def _head_train_forward(self, tpp_vecs: torch.Tensor, proj: torch.Tensor):
        """radad_model.py:39-40 in training mode (config.head_train_hip): HIP forward and backward through _FuseHeadTrainFn.
        The dropout masks (config.detection_dropout, one per hidden layer) are drawn by torch on the device under torch's
        generator, so torch.manual_seed reproduces a step; p == 0 draws nothing.  BatchNorm's bookkeeping stays here:
        num_batches_tracked goes up by one per BatchNorm after the launch, and the update factor handed to the kernel is
        bn.momentum, or 1 / num_batches_tracked (after the increment) when momentum is None.  The kernels are float32: inputs and
        parameters of another float dtype are cast up here (differentiably) and the logits are float32, as in eval.
        Returns (logits [B], fused [B,P] detached)."""
        _lib.require_cuda(tpp_vecs, "tpp_vecs")
        _lib.require_cuda(proj, "proj")
        if tpp_vecs.dim() != 2 or proj.dim() != 2 or tpp_vecs.shape[1] != self.tpp_output_dim or proj.shape[0] != tpp_vecs.shape[0] \
                or proj.shape[1] != self.fuse.out_features:
            raise ValueError(f"expected tpp [B,{self.tpp_output_dim}] and proj [B,{self.fuse.out_features}], got "
                             f"{tuple(tpp_vecs.shape)} and {tuple(proj.shape)}")
        if not (tpp_vecs.is_floating_point() and proj.is_floating_point()):
            raise TypeError(f"tpp_vecs and proj must be floating-point tensors, got {tpp_vecs.dtype} and {proj.dtype}")
        p = float(getattr(self.config, "detection_dropout", 0.1))
        if not 0.0 <= p < 1.0:
            raise ValueError(f"detection_dropout must be in [0, 1), got {p}")
        B = tpp_vecs.shape[0]
        layers = self.detection_model.head_layers()
        hidden = layers[:-1]
        bns = [bn for _, bn in hidden if bn is not None]
        if B == 1 and bns:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size "
                             f"{torch.Size([B, hidden[0][0].out_features])}")
        params = [self.fuse.weight, self.fuse.bias]
        factor, running, tmp = [], [], []
        for lin, bn in layers:
            params += [lin.weight, lin.bias]
            if lin is layers[-1][0]:
                break
            if bn is None:
                factor.append(0.0)
                running.append(None)
                continue
            params += [bn.weight, bn.bias]
            if bn.track_running_stats and bn.running_mean is not None:
                factor.append(float(bn.momentum) if bn.momentum is not None else 1.0 / (int(bn.num_batches_tracked) + 1))
                pair = (bn.running_mean, bn.running_var)
                if any(r.dtype != torch.float32 or not r.is_contiguous() for r in pair):       # a .double() module
                    pair = tuple(r.float().contiguous() for r in pair)
                    tmp.append((bn, pair))
                running.append(pair)
            else:
                factor.append(0.0)
                running.append(None)
        masks = [torch.empty((B, lin.out_features), device=tpp_vecs.device, dtype=torch.float32).bernoulli_(1.0 - p) if p > 0.0
                 else None for lin, _ in hidden]
        spec = HeadTrainSpec([bn is not None for _, bn in hidden], [bn.eps if bn is not None else 0.0 for _, bn in hidden], factor,
                             running, masks, 1.0 / (1.0 - p))
        logits, fused = _FuseHeadTrainFn.apply(tpp_vecs.float(), proj.float(), spec, *[q.float() for q in params])
        for bn, pair in tmp:
            bn.running_mean.copy_(pair[0])
            bn.running_var.copy_(pair[1])
        for bn in bns:
            if bn.track_running_stats and bn.num_batches_tracked is not None:
                bn.num_batches_tracked += 1
        return logits.squeeze(-1), fused                                       # detection_model.py:125

    def forward(self, neighbor_vecs: torch.Tensor, tpp_vecs: torch.Tensor) -> torch.Tensor:
        """radad_model.py:32-41."""
        if neighbor_vecs.device != self.device:
            neighbor_vecs = neighbor_vecs.to(self.device)
        if tpp_vecs.device != self.device:
            tpp_vecs = tpp_vecs.to(self.device)
        if not self._training_path():
            self._check_eval(neighbor_vecs, tpp_vecs)
        proj = self.projection_layer(neighbor_vecs)                            # :38
        return self.fuse_and_detect(tpp_vecs, proj)                            # :39-40

    def predict_proba(self, neighbor_vecs: torch.Tensor, tpp_vecs: torch.Tensor) -> torch.Tensor:
        """sigmoid of the logits (detection_model.py:142-155 applied to the fused model)."""
        with torch.no_grad():
            return torch.sigmoid(self.forward(neighbor_vecs, tpp_vecs))
