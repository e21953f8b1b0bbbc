"""FusedAdam: torch.optim.Adam / AdamW with the global-norm gradient clip and a non-finite guard folded in, as TWO kernel launches
per step (csrc/optim.hip: fabind_multi_sqnorm + fabind_multi_adam) and one host-to-device copy of the per-tensor table.

Replaces the tail of a training step (reference main_fabind.py:257-260 Adam / AdamW, 419-426 clip + step): `clip_grad_norm_` +
`optimizer.step()` are ~1,600 ATen launches for the 394 tensors of the production model.  The arithmetic is torch 2.10's
single-tensor Adam; hyper-parameters are read from `param_groups` on every step, so torch's LR schedulers drive it unchanged.

Differences to the torch pair, by design:
  * `.grad` is READ ONLY.  `clip_grad_norm_` rescales the gradients in place; here the clip coefficient is applied inside the update
    and `.grad` still holds the unclipped (all-reduced) gradient afterwards.  The pre-clip norm is `opt.grad_norm`.
  * a non-finite gradient norm skips the whole step on the device (`skip_nonfinite=True`): nothing is written, `opt.skipped` counts.
    No host synchronisation either way.
  * state lives in one flat fp32 buffer each for exp_avg / exp_avg_sq and one fp32 step vector; `self.state[p]` holds views of them in
    torch.optim.Adam's own format, so `state_dict()` / `load_state_dict()` interchange with torch Adam / AdamW checkpoints.

There is no CPU or eager fallback: parameters must be contiguous fp32 tensors on one HIP device."""
import numpy as np
import torch

from . import _lib
from ._lib import check, stream

CHUNK = 4096           # elements per chunk of csrc/optim.hip (FB_OPT_CHUNK; `fabind_adam_chunk()` of the built library is checked against it)

_ROW = np.dtype([("p", np.uint64), ("g", np.uint64), ("m", np.uint64), ("v", np.uint64), ("numel", np.int64), ("chunk0", np.int32),
                 ("step_idx", np.int32), ("lr", np.float64), ("beta1", np.float64), ("beta2", np.float64), ("eps", np.float64),
                 ("weight_decay", np.float64), ("decoupled", np.int32), ("pad_", np.int32)])
_UNSET = object()


def chunk_prefix(numels, chunk=CHUNK):
    """-> int64 [n + 1]: first chunk of every tensor and the total (a tensor of numel elements owns ceil(numel / chunk) chunks)."""
    n = np.asarray(numels, dtype=np.int64).reshape(-1)
    return np.concatenate([[0], np.cumsum((n + chunk - 1) // chunk)]).astype(np.int64)


def find_row(chunk0, chunk):
    """Row that owns `chunk`: the last r with chunk0[r] <= chunk -- the kernels' binary search restated on the host (tests)."""
    lo, hi = 0, len(chunk0) - 1
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if chunk0[mid] <= chunk:
            lo = mid
        else:
            hi = mid - 1
    return lo


def build_table(static, g_ptrs, hyper, chunk=CHUNK):
    """The device table of one step, on the host.
    static: structured array (_ROW) with p / m / v / numel / step_idx filled, one row per parameter tensor, and `group` = hyper row;
    g_ptrs: uint64 gradient address per row, 0 = no gradient this step; hyper: float64 [n_groups, 6] (lr, beta1, beta2, eps,
    weight_decay, decoupled).  Rows without a gradient and zero-numel rows are dropped.  -> (table, n_chunks)."""
    rows, group = static
    g_ptrs = np.asarray(g_ptrs, dtype=np.uint64)
    keep = (g_ptrs != 0) & (rows["numel"] > 0)
    t = rows[keep].copy()
    t["g"] = g_ptrs[keep]
    pre = chunk_prefix(t["numel"], chunk)
    if pre[-1] >= 2 ** 31:
        raise RuntimeError("FusedAdam: %d chunks exceed the kernels' 32-bit chunk index" % int(pre[-1]))
    t["chunk0"] = pre[:-1]
    h = np.asarray(hyper, dtype=np.float64)[group[keep]]
    for k, name in enumerate(("lr", "beta1", "beta2", "eps", "weight_decay")):
        t[name] = h[:, k]
    t["decoupled"] = h[:, 5] != 0
    return t, int(pre[-1])


class FusedAdam(torch.optim.Optimizer):
    """Adam (decoupled_weight_decay=False) / AdamW (True) on HIP, clip and non-finite skip included.

    max_grad_norm: clip the global gradient norm to this value inside the update (None: no clip); `step(max_grad_norm=...)`
    overrides it for one call.  skip_nonfinite: a step whose gradient norm is inf / NaN changes nothing and counts in `skipped`.
    `grad_norm` (0-d fp32) is the pre-clip norm of the last step, `skipped` (0-d int32) the number of skipped steps: device tensors,
    reading them is the caller's synchronisation."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False,
                 max_grad_norm=None, skip_nonfinite=True, amsgrad=False, maximize=False):
        if amsgrad or maximize:
            raise NotImplementedError("FusedAdam: amsgrad / maximize are not implemented (the reference trains with neither)")
        if torch.is_tensor(lr):
            raise NotImplementedError("FusedAdam: a tensor lr is not implemented")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("FusedAdam: invalid lr / betas / eps / weight_decay")
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = bool(skip_nonfinite)
        self._layout_key = None
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                                      decoupled_weight_decay=bool(decoupled_weight_decay), amsgrad=False, maximize=False))
        self._sync_state()

    # ---- state ---------------------------------------------------------------------------------------------------
    def _all_params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _sync_state(self):
        """(Re)build the flat state buffers for the current parameter list and point `self.state[p]` at views of them; values already
        in `self.state` (a loaded checkpoint, the previous layout) are copied in."""
        params = self._all_params()
        if not params:
            raise ValueError("FusedAdam: no parameters")
        for p in params:
            if not p.is_cuda:
                raise RuntimeError("FusedAdam needs parameters on a HIP device (there is no CPU fallback); got a %s tensor" % p.device)
            if p.dtype != torch.float32:
                raise TypeError("FusedAdam: fp32 parameters only, got %s" % p.dtype)
            if not p.is_contiguous():
                raise RuntimeError("FusedAdam: parameters must be contiguous")
        dev = params[0].device
        if any(p.device != dev for p in params):
            raise RuntimeError("FusedAdam: all parameters must live on one HIP device")
        lib = _lib.load()
        if lib.fabind_adam_chunk() != CHUNK:
            raise RuntimeError("fabind_amd.optim.CHUNK and the library's fabind_adam_chunk() disagree -- rebuild")
        key = (dev, tuple((id(p), p.numel()) for p in params))
        if key != self._layout_key:
            # (every tensor's slice starts on a 16-byte boundary of the flat buffers: the kernels' 16-byte accesses to m / v)
            offs = np.concatenate([[0], np.cumsum([(p.numel() + 3) // 4 * 4 for p in params])]).astype(np.int64)
            self._offs = offs
            self._exp_avg = torch.zeros(int(offs[-1]), dtype=torch.float32, device=dev)
            self._exp_avg_sq = torch.zeros(int(offs[-1]), dtype=torch.float32, device=dev)
            self._steps = torch.zeros(len(params), dtype=torch.float32, device=dev)
            n_chunks = int(chunk_prefix([p.numel() for p in params])[-1])
            self._partials = torch.zeros(max(1, n_chunks), dtype=torch.float32, device=dev)
            self._snap = torch.zeros(len(params), dtype=torch.float32, device=dev)
            self.grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
            if getattr(self, "skipped", None) is None or self.skipped.device != dev:
                self.skipped = torch.zeros((), dtype=torch.int32, device=dev)
            self._layout_key = key
        self._params, self._device = params, dev
        step_idx, step_val = [], []
        with torch.no_grad():
            for i, p in enumerate(params):
                lo, n = int(self._offs[i]), p.numel()
                m, v, s = self._exp_avg[lo:lo + n].view_as(p), self._exp_avg_sq[lo:lo + n].view_as(p), self._steps[i]
                old = self.state.get(p)
                if old:
                    m.copy_(old["exp_avg"])
                    v.copy_(old["exp_avg_sq"])
                    st = old["step"]
                    if not (torch.is_tensor(st) and st.is_cuda and st.data_ptr() == s.data_ptr()):      # (else: already in place)
                        step_idx.append(i)
                        step_val.append(float(st))
                self.state[p] = {"step": s, "exp_avg": m, "exp_avg_sq": v}
            if step_idx:
                self._steps.index_copy_(0, torch.tensor(step_idx, dtype=torch.int64).to(dev), torch.tensor(step_val, dtype=torch.float32).to(dev))
        # static part of the table (addresses of p / m / v, sizes, group of every row); the gradient addresses and the
        # hyper-parameters are filled in per step
        rows = np.zeros(len(params), dtype=_ROW)
        esz = 4
        rows["p"] = [p.data_ptr() for p in params]
        rows["m"] = self._exp_avg.data_ptr() + self._offs[:-1] * esz
        rows["v"] = self._exp_avg_sq.data_ptr() + self._offs[:-1] * esz
        rows["numel"] = [p.numel() for p in params]
        rows["step_idx"] = np.arange(len(params))
        group = np.concatenate([np.full(len(g["params"]), k, dtype=np.int64) for k, g in enumerate(self.param_groups)])
        self._static = (rows, group)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if getattr(self, "_layout_key", None) is not None:          # (the constructor syncs once, after all groups)
            self._sync_state()

    def load_state_dict(self, state_dict):
        """Accepts a FusedAdam or a torch.optim.Adam / AdamW state dict: the values are copied into the flat buffers and
        `self.state[p]` is again a set of views of them."""
        super().load_state_dict(state_dict)
        self._sync_state()

    # ---- step ----------------------------------------------------------------------------------------------------
    def _hyper(self):
        h = np.zeros((len(self.param_groups), 6), dtype=np.float64)
        for k, g in enumerate(self.param_groups):
            if g.get("amsgrad") or g.get("maximize"):
                raise NotImplementedError("FusedAdam: amsgrad / maximize are not implemented")
            if torch.is_tensor(g["lr"]):
                raise NotImplementedError("FusedAdam: a tensor lr is not implemented")
            h[k] = (g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], 1.0 if g.get("decoupled_weight_decay") else 0.0)
        return h

    @torch.no_grad()
    def step(self, closure=None, max_grad_norm=_UNSET):
        """One Adam / AdamW step on every parameter that has a gradient (a parameter whose .grad is None gets no update, no decay and
        no step increment, as in torch).  max_grad_norm: this call's clip norm (None: no clip); default: the constructor's."""
        if closure is not None:
            raise NotImplementedError("FusedAdam: a closure is not implemented")
        from . import param_pack
        params = self._params
        rows, _ = self._static
        if len(params) != sum(len(g["params"]) for g in self.param_groups) or \
                any(p.data_ptr() != a for p, a in zip(params, rows["p"].tolist())):
            self._sync_state()                                   # a parameter's storage was replaced (module.to(), p.data = ...)
            params = self._params
        g_ptrs = np.zeros(len(params), dtype=np.uint64)
        touched = []
        for i, p in enumerate(params):
            g = p.grad
            if g is None:
                continue
            if g.dtype != torch.float32 or g.device != self._device or g.layout != torch.strided:
                raise TypeError("FusedAdam: gradients must be dense fp32 tensors on %s, got %s on %s" % (self._device, g.dtype, g.device))
            if not g.is_contiguous():
                raise RuntimeError("FusedAdam: gradients must be contiguous")
            g_ptrs[i] = g.data_ptr()
            touched.append(p)
        table, n_chunks = build_table(self._static, g_ptrs, self._hyper())
        if len(table) == 0:
            return None
        clip = self.max_grad_norm if max_grad_norm is _UNSET else max_grad_norm
        flags = (1 if clip is not None else 0) | (2 if self.skip_nonfinite else 0)
        tdev = param_pack._upload(table, self._device)            # pinned ring: asynchronous, no stream drain
        lib, s = _lib.load(), stream()
        check(lib.fabind_multi_sqnorm(tdev.data_ptr(), len(table), n_chunks, self._steps.data_ptr(), self._partials.data_ptr(),
                                      self._snap.data_ptr(), s), "fabind_multi_sqnorm")
        check(lib.fabind_multi_adam(tdev.data_ptr(), len(table), n_chunks, self._partials.data_ptr(), self._snap.data_ptr(),
                                    self._steps.data_ptr(), float(clip) if clip is not None else 0.0, flags, self.grad_norm.data_ptr(),
                                    self.skipped.data_ptr(), s), "fabind_multi_adam")
        # the kernels wrote through raw pointers: without this, caches keyed on (data_ptr, _version) -- engine.cached_pack's no-grad
        # parameter pack -- would keep serving the old weights
        torch.autograd.graph.increment_version(touched)
        return None
