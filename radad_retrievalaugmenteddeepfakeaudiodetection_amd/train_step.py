"""HipTrainStep -- what RADAD's training loop does after the forward (pipeline.py:815-836) in four HIP launches and no host
round trip (csrc/optim_step.inc): BCEWithLogitsLoss(pos_weight) with its gradient and the accuracy count, GradScaler.unscale_,
clip_grad_norm_ and torch.optim.Adam per optimizer, GradScaler.step's skip and GradScaler.update.

    step = HipTrainStep.for_model(radad_model, config, pos_weight)      # pipeline.py:96-109, 768-770
    logits = radad_model(vecs, tpp)
    step.zero_grad()
    loss, correct = step.backward(logits, labels)                       # :815, :820, :835-836 -- device tensors
    step.step()                                                         # :822-832
    s = step.stats()                                                    # the one host read: loss, correct, grad_norms, scale, ...

Everything the loop logs (loss, correct count, the gradient norms, the scale) stays on the device until stats() is called.
The hyperparameters travel as float32 (radad_optim_group): `hyper` holds the values in use, e.g. beta2 = 0.999 is
0.9990000128746033.  There is no CPU fallback: the tensors must live on one ROCm device.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

_HYPER = ("lr", "beta1", "beta2", "eps", "weight_decay", "max_norm")


def _f32(v):
    return float(np.float32(v))


def _per_group(value, n, name):
    """A scalar for every group, or one value per group."""
    if isinstance(value, (list, tuple)) and name != "betas":
        if len(value) != n:
            raise ValueError(f"{name}: {len(value)} values for {n} groups")
        return list(value)
    if name == "betas" and len(value) > 0 and isinstance(value[0], (list, tuple)):
        if len(value) != n:
            raise ValueError(f"betas: {len(value)} pairs for {n} groups")
        return [tuple(b) for b in value]
    return [value] * n


def check_groups(groups):
    """TypeError / ValueError unless `groups` is what the kernels can index through raw pointers: at most OPTIM_MAX_GROUPS lists
    of, in all, at most OPTIM_MAX_TENSORS distinct contiguous float32 tensors on one ROCm device.  Returns [[tensor]]."""
    groups = [list(g) for g in groups]
    if not 1 <= len(groups) <= _lib.OPTIM_MAX_GROUPS:
        raise ValueError(f"HipTrainStep: {len(groups)} groups, need 1..{_lib.OPTIM_MAX_GROUPS}")
    flat = [p for g in groups for p in g]
    for p in flat:
        if not isinstance(p, torch.Tensor):
            raise TypeError(f"HipTrainStep: parameters must be tensors, got {type(p).__name__}")
        if p.dtype != torch.float32:
            raise TypeError(f"HipTrainStep: parameters must be float32 (the kernels are float32), got {p.dtype}")
    if len(flat) > _lib.OPTIM_MAX_TENSORS:
        raise ValueError(f"HipTrainStep: {len(flat)} tensors, at most {_lib.OPTIM_MAX_TENSORS} per step")
    if len({id(p) for p in flat}) != len(flat):
        raise ValueError("HipTrainStep: a parameter appears in more than one group")
    for p in flat:
        if not p.is_contiguous():
            raise ValueError(f"HipTrainStep: parameters must be contiguous (they are updated in place), got strides {p.stride()} "
                             f"for shape {tuple(p.shape)}")
    if len({p.device for p in flat}) > 1:
        raise ValueError(f"HipTrainStep: all tensors must sit on one device, got {sorted({str(p.device) for p in flat})}")
    if flat and not flat[0].is_cuda:
        raise ValueError(f"HipTrainStep: parameters must be on a ROCm device, got {flat[0].device}: there is no CPU fallback")
    return groups


def check_hyper(n_groups, lr, weight_decay, betas, eps, max_norm, pos_weight, init_scale, growth_factor, backoff_factor,
                growth_interval):
    """ValueError for what torch.optim.Adam, BCEWithLogitsLoss and GradScaler refuse; returns one dict of float32-valued
    hyperparameters per group."""
    lrs, wds, bts = _per_group(lr, n_groups, "lr"), _per_group(weight_decay, n_groups, "weight_decay"), _per_group(betas, n_groups, "betas")
    epss, mxs = _per_group(eps, n_groups, "eps"), _per_group(max_norm, n_groups, "max_norm")
    hyper = []
    for i in range(n_groups):
        h = dict(lr=_f32(lrs[i]), beta1=_f32(bts[i][0]), beta2=_f32(bts[i][1]), eps=_f32(epss[i]), weight_decay=_f32(wds[i]),
                 max_norm=_f32(mxs[i] if mxs[i] is not None else 0.0))
        if not h["lr"] >= 0.0:
            raise ValueError(f"Invalid learning rate: {lrs[i]}")
        if not h["eps"] > 0.0:
            raise ValueError(f"Invalid epsilon value: {epss[i]} (must be positive, and at least 1.5e-45 to be a float32)")
        if not 0.0 <= h["beta1"] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {bts[i][0]}")
        if not 0.0 <= h["beta2"] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {bts[i][1]}")
        if not h["weight_decay"] >= 0.0:
            raise ValueError(f"Invalid weight_decay value: {wds[i]}")
        if h["max_norm"] != h["max_norm"]:
            raise ValueError("max_norm is not a number")
        hyper.append(h)
    if not float(pos_weight) > 0.0:
        raise ValueError(f"pos_weight must be positive, got {pos_weight}")
    if not float(init_scale) > 0.0:
        raise ValueError(f"init_scale must be positive, got {init_scale}")
    if not float(growth_factor) >= 1.0:
        raise ValueError(f"growth_factor must be at least 1, got {growth_factor}")
    if not 0.0 < float(backoff_factor) <= 1.0:
        raise ValueError(f"backoff_factor must be in (0, 1], got {backoff_factor}")
    if int(growth_interval) < 1:
        raise ValueError(f"growth_interval must be at least 1, got {growth_interval}")
    return hyper


def check_logits(logits, labels, device):
    """TypeError / ValueError unless backward() can hand `logits` to the loss kernel."""
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32:
        raise TypeError(f"logits must be a float32 tensor, got {getattr(logits, 'dtype', type(logits).__name__)}")
    if not isinstance(labels, torch.Tensor):
        raise TypeError(f"labels must be a tensor, got {type(labels).__name__}")
    if logits.device != device:
        raise ValueError(f"logits are on {logits.device}, the parameters on {device}")
    if labels.numel() != logits.numel() or logits.numel() == 0:
        raise ValueError(f"logits {tuple(logits.shape)} and labels {tuple(labels.shape)} must have the same, non-zero, number of "
                         f"elements")


def check_grad(p, g, device):
    """TypeError / ValueError unless step() can take the raw pointers of parameter `p` and its gradient `g`."""
    if g.dtype != torch.float32:
        raise TypeError(f"gradients must be float32, got {g.dtype}")
    if g.device != device or p.device != device:
        raise ValueError(f"a parameter or its gradient left {device} ({p.device}, {g.device})")
    if not p.is_contiguous():
        raise ValueError("parameters must be contiguous (they are updated in place)")


class HipTrainStep:
    """`groups`: a list of parameter iterables, one per optimizer of the reference.  lr, weight_decay, eps, max_norm: one value,
    or one per group; betas: one pair, or one pair per group.  max_norm None or <= 0: the norm is reported, nothing is clipped.
    loss_scaling=False: no GradScaler (scale() stays 1, nothing is ever skipped)."""

    def __init__(self, groups, lr, weight_decay, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0, pos_weight=1.0, init_scale=65536.0,
                 growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, loss_scaling=True):
        self.groups = check_groups(groups)
        G = len(self.groups)
        self.hyper = check_hyper(G, lr, weight_decay, betas, eps, max_norm, pos_weight, init_scale, growth_factor, backoff_factor,
                                 growth_interval)
        self.pos_weight = float(pos_weight)
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self.loss_scaling = bool(loss_scaling)
        self._flat = [(p, gi) for gi, g in enumerate(self.groups) for p in g]
        if not self._flat:
            raise ValueError("HipTrainStep: no parameters")
        self.device = self._flat[0][0].device
        self._lib = _lib.load()
        self.exp_avg = [[torch.zeros_like(p, memory_format=torch.contiguous_format).detach() for p in g] for g in self.groups]
        self.exp_avg_sq = [[torch.zeros_like(p, memory_format=torch.contiguous_format).detach() for p in g] for g in self.groups]
        # one block of 4-byte slots, so that stats() is one read: scale, growth_tracker, loss, correct, then per group
        # grad_norm, found_inf, steps (float32 or int32 as the kernels write them)
        self._state = torch.zeros(4 + 3 * G, dtype=torch.float32, device=self.device)
        self._state_i = self._state.view(torch.int32)
        self._state[0] = float(init_scale) if self.loss_scaling else 1.0
        self._o_norm, self._o_found, self._o_steps = 4, 4 + G, 4 + 2 * G
        numels = (C.c_int64 * len(self._flat))(*[p.numel() for p, _ in self._flat])
        need = self._lib.radad_optim_workspace_bytes(numels, len(self._flat))
        if need < 0:
            raise ValueError("HipTrainStep: the parameters are outside the kernels' limits")
        self._ws = torch.empty(int(need), dtype=torch.uint8, device=self.device)
        self._tensors = (_lib.OptimTensor * len(self._flat))()
        moments = [(m, v) for gm, gv in zip(self.exp_avg, self.exp_avg_sq) for m, v in zip(gm, gv)]
        for t, (p, gi), (m, v) in zip(self._tensors, self._flat, moments):
            t.exp_avg, t.exp_avg_sq, t.numel, t.group = m.data_ptr(), v.data_ptr(), p.numel(), gi
        self._groups_c = (_lib.OptimGroup * G)()
        for c, h in zip(self._groups_c, self.hyper):
            for k in _HYPER:
                setattr(c, k, h[k])
        base = self._state.data_ptr()
        self._state_c = _lib.OptimState()
        if self.loss_scaling:
            self._state_c.scale, self._state_c.growth_tracker = base, base + 4
        self._state_c.grad_norm, self._state_c.found_inf = base + 4 * self._o_norm, base + 4 * self._o_found
        self._state_c.steps = base + 4 * self._o_steps

    @classmethod
    def for_model(cls, radad_model, config, pos_weight, **kwargs):
        """The reference's configuration: three Adam optimizers over projection_layer, fuse and detection_model with
        config.learning_rate / config.weight_decay (pipeline.py:96-107; config.py:68-69 where the config has no such key),
        clip_grad_norm_ at 1.0 (:825-827), GradScaler's defaults (:109), BCEWithLogitsLoss(pos_weight) (:768-770)."""
        groups = [radad_model.projection_layer.parameters(), radad_model.fuse.parameters(), radad_model.detection_model.parameters()]
        return cls(groups, lr=getattr(config, "learning_rate", 1e-3), weight_decay=getattr(config, "weight_decay", 1e-5),
                   max_norm=1.0, pos_weight=pos_weight, **kwargs)

    # ---- the step ------------------------------------------------------------------------------------------------------
    def zero_grad(self):
        """optimizer.zero_grad() x3 (pipeline.py:817-819): gradients go to None."""
        for p, _ in self._flat:
            p.grad = None

    def backward(self, logits, labels):
        """criterion(logits, labels) and scaler.scale(loss).backward() (pipeline.py:815, 820) in one launch plus autograd's
        backward from the logits.  Returns (loss, correct): the unscaled mean loss [float32 scalar] and the count of
        (logits > 0) == labels [int32 scalar] (:835-836), device tensors, no synchronisation.  Both are views of this object's
        state block: the next backward() overwrites them."""
        check_logits(logits, labels, self.device)
        x = logits.detach().contiguous()
        y = labels.detach().to(device=self.device, dtype=torch.float32).contiguous()
        dlogits = torch.empty_like(x)
        base = self._state.data_ptr()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.radad_bce_logits(x.data_ptr(), y.data_ptr(), x.numel(), self.pos_weight,
                                                  base if self.loss_scaling else None, base + 8, dlogits.data_ptr(), base + 12,
                                                  self.device.index, _lib.stream_ptr(self.device)), "radad_bce_logits")
        logits.backward(dlogits.view_as(logits))
        return self._state[2], self._state_i[3]

    def step(self):
        """unscale_, clip_grad_norm_, scaler.step per group and scaler.update (pipeline.py:822-832) in one radad_optim_step call.
        A parameter whose .grad is None takes no part.  Whether a group was skipped for a non-finite gradient is decided on the
        device; every parameter that had a gradient gets its _version bumped either way, so caches keyed on it
        (ProjectionLayer's fold) see the update as they do after a torch optimizer."""
        touched = []
        for t, (p, _) in zip(self._tensors, self._flat):
            g = p.grad
            if g is None:
                t.grad = None
                continue
            check_grad(p, g, self.device)
            if not g.is_contiguous():
                g = g.contiguous()
                p.grad = g
            t.param, t.grad = p.data_ptr(), g.data_ptr()
            touched.append(p)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.radad_optim_step(self._tensors, len(self._tensors), self._groups_c, len(self._groups_c),
                                                  C.byref(self._state_c), self.growth_factor, self.backoff_factor,
                                                  self.growth_interval, self._ws.data_ptr(), int(self._ws.numel()),
                                                  self.device.index, _lib.stream_ptr(self.device)), "radad_optim_step")
        if touched:
            torch.autograd.graph.increment_version(touched)

    # ---- what the loop logs, on the device ------------------------------------------------------------------------------
    def grad_norms(self):
        """[n_groups] float32: the norms clip_grad_norm_ returned in the last step()."""
        return self._state[self._o_norm:self._o_found]

    def steps(self):
        """[n_groups] int32: Adam's step count per group."""
        return self._state_i[self._o_steps:]

    def scale(self):
        """float32 scalar: GradScaler's scale (1 without loss scaling)."""
        return self._state[0]

    def stats(self):
        """One device-to-host copy of everything pipeline.py:825-836 reads per step."""
        h = self._state.cpu().numpy()
        hi = h.view(np.int32)
        return {"loss": float(h[2]), "correct": int(hi[3]), "grad_norms": [float(v) for v in h[self._o_norm:self._o_found]],
                "found_inf": [int(v) for v in hi[self._o_found:self._o_steps]], "steps": [int(v) for v in hi[self._o_steps:]],
                "scale": float(h[0]), "growth_tracker": int(hi[1])}

    # ---- checkpoints ----------------------------------------------------------------------------------------------------
    def state_dict(self):
        return {"exp_avg": [[m.clone() for m in g] for g in self.exp_avg], "exp_avg_sq": [[v.clone() for v in g] for g in self.exp_avg_sq],
                "steps": self.steps().clone(), "scale": self.scale().clone(), "growth_tracker": self._state_i[1].clone()}

    def load_state_dict(self, sd):
        shapes = lambda gs: [[tuple(t.shape) for t in g] for g in gs]
        for k in ("exp_avg", "exp_avg_sq"):
            if shapes(sd[k]) != shapes(self.groups):
                raise ValueError(f"load_state_dict: {k} does not match the parameters' shapes")
        if sd["steps"].numel() != len(self.groups):
            raise ValueError(f"load_state_dict: {sd['steps'].numel()} step counts for {len(self.groups)} groups")
        with torch.no_grad():
            for k, mine in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
                for gm, gs in zip(mine, sd[k]):
                    for m, s in zip(gm, gs):
                        m.copy_(s)
            self._state_i[self._o_steps:].copy_(sd["steps"].to(torch.int32))
            self._state[0].copy_(sd["scale"].to(torch.float32))
            self._state_i[1].copy_(sd["growth_tracker"].to(torch.int32))
