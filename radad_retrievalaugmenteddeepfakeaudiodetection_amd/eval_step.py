"""HipEvalMetrics -- RADAD's validation pass behind the forward (pipeline.py:725-733) and the metrics train() / evaluate()
compute from it (pipeline.py:868-872, 983-987), on the device (csrc/eval_metrics.inc): every batch is appended to device buffers
in one launch with no host read; compute() returns every number the reference logs in one device-to-host copy.

    ev = HipEvalMetrics(pos_weight, device, asv_params=getattr(config, "asv_params", None))
    ev.reset()
    for batch in loader:                                   # pipeline.py:711-752
        logits = radad_model(vecs, tpp)
        ev.add(logits, lbls, speakers)                     # :725-741 -- speakers: list of str, an int tensor, or None
    m = ev.compute()                                       # :754-755, :868-872 -- the one host read
    m = ev.compute(curves=True)                            # the same, and keeps the curves on the device for:
    fpr, tpr, thr = ev.roc_points()                        # what _plot_and_save_roc_det writes to its CSV

m holds loss, acc, n, auc, eer_percent, eer_threshold, macro_eer_percent, groups_scored, min_tDCF, min_tDCF_threshold and
nonfinite.  On tied scores the AUC and the ROC points take the counts at the end of each run of equal scores (the usual
definition); the reference keeps an arbitrary element of the run.  There is no CPU fallback.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

ASV_KEYS = ("P_miss_asv", "P_fa_asv", "P_fa_spoof_asv", "C_miss_asv", "C_fa_asv", "C_miss_cm", "C_fa_cm", "pi_tar", "pi_non",
            "pi_spoof")
_ACC = _lib.EVAL_ACC_BYTES // 8


def tdcf_consts(asv_params):
    """The constants of pipeline.py:303-323 as Python floats in the reference's left-to-right order, or None where the reference
    returns NaN (no asv_params, C_def <= 0).  ValueError unless asv_params is None or carries the reference's ten keys."""
    if asv_params is None:
        return None
    missing = [k for k in ASV_KEYS if k not in asv_params]
    if missing:
        raise ValueError(f"asv_params lacks {missing}: it must carry {list(ASV_KEYS)} or be None")
    a = {k: float(asv_params[k]) for k in ASV_KEYS}
    c_def = min(a["C_miss_asv"] * a["pi_tar"], a["C_fa_asv"] * a["pi_non"])
    if not c_def > 0:
        return None
    c = _lib.TdcfConsts()
    c.c0 = a["C_miss_asv"] * a["pi_tar"] * a["P_miss_asv"] + a["C_fa_asv"] * a["pi_non"] * a["P_fa_asv"]
    c.c1 = a["C_fa_cm"] * a["pi_spoof"]
    c.c2 = a["C_miss_cm"] * a["pi_tar"]
    c.p_fa_spoof_asv = a["P_fa_spoof_asv"]
    c.c_def = c_def
    return c


def check_batch(logits, labels, speakers, device):
    """TypeError / ValueError unless add() can hand the batch to the append kernel.  Returns the number of samples."""
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32:
        raise TypeError(f"logits must be a float32 tensor, got {getattr(logits, 'dtype', type(logits).__name__)}")
    if not isinstance(labels, torch.Tensor):
        raise TypeError(f"labels must be a tensor, got {type(labels).__name__}")
    if logits.device != device:
        raise ValueError(f"logits are on {logits.device}, the metrics on {device}: there is no CPU fallback")
    n = logits.numel()
    if labels.numel() != n or n == 0:
        raise ValueError(f"logits {tuple(logits.shape)} and labels {tuple(labels.shape)} must have the same, non-zero, number of "
                         f"elements")
    if speakers is None:
        return n
    if isinstance(speakers, torch.Tensor):
        if speakers.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"a speakers tensor must be int32 or int64 (dense group ids in 0 .. 2^31 - 1), got {speakers.dtype}")
        if speakers.numel() != n:
            raise ValueError(f"{speakers.numel()} speakers for {n} logits")
        return n
    if not isinstance(speakers, (list, tuple)):
        raise TypeError(f"speakers must be a list of str, an int tensor or None, got {type(speakers).__name__}")
    if len(speakers) != n:
        raise ValueError(f"{len(speakers)} speakers for {n} logits")
    for s in speakers:
        if not isinstance(s, str):
            raise TypeError(f"speakers must be str, got {type(s).__name__}")
    return n


class HipEvalMetrics:
    """`capacity`: samples the buffers hold at first; they grow by doubling (a device copy) up to EVAL_MAX_N.  Samples without
    speakers (speakers=None) belong to group 0, which is also the id of the first speaker name seen: mix the two forms only if
    that is meant.  Ids given as an int tensor must lie in 0 .. 2^31 - 1: they are not read back to be checked, the key holds
    their low 31 bits, and an id outside that range lands in another id's group."""

    def __init__(self, pos_weight, device, asv_params=None, capacity=65536):
        if not float(pos_weight) > 0.0:
            raise ValueError(f"pos_weight must be positive, got {pos_weight}")
        if not 1 <= int(capacity) <= _lib.EVAL_MAX_N:
            raise ValueError(f"capacity must be in 1..{_lib.EVAL_MAX_N}, got {capacity}")
        self._consts = tdcf_consts(asv_params)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"HipEvalMetrics needs a ROCm device, got {self.device}: there is no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.pos_weight = float(np.float32(pos_weight))          # travels as float32, like BCEWithLogitsLoss's own tensor
        self._lib = _lib.load()
        self._cap = int(capacity)
        self._keys = torch.empty(self._cap, dtype=torch.int64, device=self.device)
        self._scores = torch.empty(self._cap, dtype=torch.float32, device=self.device)
        self._labels = torch.empty(self._cap, dtype=torch.float32, device=self.device)
        # one block of 8-byte slots, so that compute() is one read: the four accumulators, then radad_eval_metrics' out
        self._state = torch.zeros(_ACC + _lib.EVAL_OUT_DOUBLES, dtype=torch.float64, device=self.device)
        self._ws = None
        self.reset()

    def reset(self):
        """A new validation pass: no samples, no speakers.  No synchronisation."""
        self._n = 0
        self._ids = {}
        self._has_groups = False
        self._curves = None
        self._state.zero_()

    def __len__(self):
        return self._n

    def _grow(self, need):
        if need > _lib.EVAL_MAX_N:
            raise ValueError(f"{need} samples: one pass holds at most {_lib.EVAL_MAX_N}")
        cap = self._cap
        while cap < need:
            cap = min(2 * cap, _lib.EVAL_MAX_N)
        for name in ("_keys", "_scores", "_labels"):
            old = getattr(self, name)
            new = torch.empty(cap, dtype=old.dtype, device=self.device)
            new[:self._n].copy_(old[:self._n])
            setattr(self, name, new)
        self._cap = cap

    def _to_device(self, t, dtype):
        """`t` flat on the device as `dtype`, without making the host wait: a host tensor is staged through pinned memory (the
        caching host allocator keeps the block until the copy has run) and copied with non_blocking=True."""
        t = t.detach().reshape(-1)
        if t.device == self.device:
            return t.to(dtype)
        return t.to(dtype).pin_memory().to(self.device, non_blocking=True)

    def add(self, logits, labels, speakers=None):
        """One validation batch (pipeline.py:725-741): one radad_eval_append launch behind the copies into this object's
        buffers.  Nothing is read back and the host never waits for the device: labels or speaker ids that live on the host
        (the loader's int64 labels, name lists mapped to dense ids in a dict this object keeps until reset()) are staged
        through pinned memory and copied asynchronously on the current stream."""
        n = check_batch(logits, labels, speakers, self.device)
        if self._n + n > self._cap:
            self._grow(self._n + n)
        lo, hi = self._n, self._n + n
        self._curves = None
        self._scores[lo:hi].copy_(logits.detach().reshape(-1))
        self._labels[lo:hi].copy_(self._to_device(labels, torch.float32))
        gid = None
        if isinstance(speakers, torch.Tensor):
            gid = self._to_device(speakers, torch.int32).contiguous()
            self._has_groups = True
        elif speakers is not None:
            ids = self._ids
            gid = self._to_device(torch.tensor([ids.setdefault(s, len(ids)) for s in speakers], dtype=torch.int32), torch.int32)
            self._has_groups = self._has_groups or len(ids) > 1
        with torch.cuda.device(self.device):
            _lib.check(self._lib.radad_eval_append(self._scores.data_ptr() + 4 * lo, self._labels.data_ptr() + 4 * lo,
                                                   gid.data_ptr() if gid is not None else None, n, self.pos_weight, lo,
                                                   self._keys.data_ptr(), self._state.data_ptr(), self.device.index,
                                                   _lib.stream_ptr(self.device)), "radad_eval_append")
        self._n = hi

    def scores(self):
        """[n] float32: the logits in arrival order, a device view."""
        return self._scores[:self._n]

    def labels(self):
        """[n] float32: the labels in arrival order, a device view."""
        return self._labels[:self._n]

    def _metrics(self, roc, geer):
        if self._n == 0:
            raise ValueError("HipEvalMetrics: no samples since reset()")
        groups = int(self._has_groups)
        need = int(self._lib.radad_eval_metrics_workspace_bytes(self._n, groups))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.radad_eval_metrics(self._keys.data_ptr(), self._n, groups,
                                                    C.byref(self._consts) if self._consts is not None else None,
                                                    self._state.data_ptr() + 8 * _ACC, roc.data_ptr() if roc is not None else None,
                                                    geer.data_ptr() if geer is not None else None,
                                                    self._ws.data_ptr(), int(self._ws.numel()), self.device.index,
                                                    _lib.stream_ptr(self.device)), "radad_eval_metrics")

    def compute(self, curves=False):
        """Everything pipeline.py:754-755 and :868-872 produce, in one device-to-host copy.  May be called again, also after
        more add()s.  curves=True: the same call also leaves the ROC points and the groups' EERs on the device, so that
        roc_points() and group_eers() behind it cost one copy each and no second pass."""
        roc = geer = None
        if curves:
            roc = torch.empty(3 * (self._n + 2), dtype=torch.float64, device=self.device)
            geer = torch.empty(self._n, dtype=torch.float64, device=self.device)
        self._metrics(roc, geer)
        h = self._state.cpu().numpy()
        acc_i = h[:_ACC].view(np.int64)
        out = dict(zip(_lib.EVAL_OUT, (float(v) for v in h[_ACC:])))
        count = int(acc_i[2])
        m = {"loss": float(h[0]) / max(count, 1), "acc": int(acc_i[1]) / max(count, 1), "n": count, "correct": int(acc_i[1]),
             "nonfinite": int(acc_i[3])}
        for k in ("auc", "eer_percent", "eer_threshold", "macro_eer_percent", "min_tDCF", "min_tDCF_threshold"):
            m[k] = out[k]
        for k in ("groups_scored", "positives", "negatives", "distinct"):
            m[k] = int(out[k])
        if curves:
            self._curves = (roc.view(3, self._n + 2)[:, :int(out["roc_points"])], geer[:m["groups_scored"]])
        return m

    def roc_points(self):
        """(fpr, tpr, thresholds) as float64 numpy arrays: _roc_curve's outputs (pipeline.py:196-229), the columns
        _plot_and_save_roc_det (:619) writes to its CSV.  One copy behind compute(curves=True); otherwise it runs that first."""
        if self._curves is None:
            self.compute(curves=True)
        r = self._curves[0].cpu().numpy()
        return r[0].copy(), r[1].copy(), r[2].copy()

    def group_eers(self):
        """float64 numpy array: the EER (percent) of every group that holds both classes, in ascending group id (ids of speaker
        names: order of first appearance) -- the terms of macro_eer_percent.  One copy behind compute(curves=True)."""
        if self._curves is None:
            self.compute(curves=True)
        return self._curves[1].cpu().numpy()
