"""`FusedOptimizer`: gradient clipping and the Adam / SGD-momentum update of ALL parameters of an optimiser in two kernel
launches (`csrc/pcc_optim.hip`) -- what `train.py:224-227` of the reference does with `clip_grad_norm_` over ~77 small
tensors and `optim.Adam` / `optim.SGD(momentum=0.9)`.

Arithmetic (restated in float64 by `tests/optim_ref.py`): the total norm is the square root of an fp64 sum of g * g in a
fixed order, coef = min(1, max_norm / (norm + 1e-6)); Adam in torch's default form (no amsgrad, no weight decay), SGD with
`buf = g` on a tensor's first step and `buf = momentum * buf + g` after it.  Equal inputs give equal bits.

What differs from torch:
* the gradients are NOT overwritten with the clipped values (`clip_grad_norm_` does overwrite them): `p.grad` after
  `step()` is what backward left there.  The norm of the step is in `last_norm` (a device scalar; nothing is read back).
* the state tensors are views into two flat buffers owned by the optimiser (every tensor's offset 16-byte aligned);
  `state[p]` shows them under torch's names (`step`, `exp_avg`, `exp_avg_sq`, `momentum_buffer`), `state_dict()` returns
  copies in the layout of `torch.optim.Adam` / `SGD`, and `load_state_dict` takes a state dict written by either -- a
  checkpoint of the reference's `train.py` resumes here and the reverse.
* one parameter group.  `lr` is read from it on every step, so `StepLR` works unchanged.

Per step: at most two launches and one small host->device copy (the segment table: the gradient pointers change whenever
gradients are set to None, and every tensor's own step count travels with them), no device->host read.  A raw kernel write
does not touch a tensor's version counter, and every packed-weight cache of this package is keyed on
`(data_ptr, _version)`, so `step()` ends with `torch.autograd.graph.increment_version` on the tensors it wrote.
"""
import numpy as np
import torch

from . import lib as L

PccError = L.PccError

ADAM, SGD = 0, 1                    # PCC_OPTIM_ADAM / PCC_OPTIM_SGD
SEG_WORDS = 6                       # PCC_OPTIM_SEG_WORDS: param*, grad*, state1*, state2*, n, t
_ALIGN = 4                          # fp32 elements per 16 bytes


def _torch_defaults(mode, lr, betas, eps, momentum):
    """The `defaults` of the torch optimiser this one stands in for, keys as the installed torch names them: a state dict
    written here then loads into `torch.optim.Adam` / `SGD` with every key they read."""
    probe = [torch.zeros(1)]
    if mode == "adam":
        return dict(torch.optim.Adam(probe, lr=lr, betas=betas, eps=eps).defaults)
    return dict(torch.optim.SGD(probe, lr=lr, momentum=momentum).defaults)


class FusedOptimizer(torch.optim.Optimizer):
    def __init__(self, params, lr, mode="adam", betas=(0.9, 0.999), eps=1e-8, momentum=0.9, max_norm=None):
        if mode not in ("adam", "sgd"):
            raise ValueError(f"mode is 'adam' or 'sgd', not {mode!r}")
        if not lr >= 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if max_norm is not None and not float(max_norm) > 0.0:
            raise ValueError(f"max_norm must be positive or None, not {max_norm}")
        self.mode, self.max_norm = mode, (None if max_norm is None else float(max_norm))
        self._ready = False
        super().__init__(params, _torch_defaults(mode, lr, tuple(betas), eps, momentum))
        if len(self.param_groups) != 1:
            raise PccError("FusedOptimizer takes one parameter group")
        ps = self.param_groups[0]["params"]
        if not ps:
            raise ValueError("optimizer got an empty parameter list")
        for i, p in enumerate(ps):
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.device != ps[0].device:
                raise PccError(f"FusedOptimizer: parameter {i} must be a contiguous float32 tensor on one GPU (no CPU fallback); "
                               f"got {p.dtype}, {p.device}, contiguous={p.is_contiguous()}")
        self._params, self.device = ps, ps[0].device
        sizes = np.array([p.numel() for p in ps], dtype=np.int64)
        offs = np.zeros(len(ps) + 1, dtype=np.int64)
        offs[1:] = np.cumsum((sizes + _ALIGN - 1) // _ALIGN * _ALIGN)         # every tensor starts on a 16-byte boundary
        self._offsets = offs
        total = max(int(offs[-1]), _ALIGN)
        self._flat1 = torch.zeros(total, dtype=torch.float32, device=self.device)
        self._flat2 = torch.zeros(total, dtype=torch.float32, device=self.device) if mode == "adam" else None
        self._steps = torch.zeros(len(ps), dtype=torch.float32)              # state[p]["step"] are views of it (CPU, as torch's)
        self._steps_np = self._steps.numpy()
        lib = L.load()
        self._n_chunks = int(lib.pcc_optim_build_chunks(L.nptr(sizes), len(ps), None, 0))
        if self._n_chunks < 0:
            raise PccError("FusedOptimizer: too many elements for one chunk table")
        chunks = np.zeros((max(self._n_chunks, 1), 2), dtype=np.int32)
        lib.pcc_optim_build_chunks(L.nptr(sizes), len(ps), L.nptr(chunks), self._n_chunks)
        self._chunks = torch.from_numpy(chunks).to(self.device)
        self._ws_bytes = int(lib.pcc_optim_ws_bytes(self._n_chunks))
        self._partials = torch.zeros(self._ws_bytes // 8, dtype=torch.float64, device=self.device)
        self.last_norm = torch.zeros((), dtype=torch.float32, device=self.device)
        # the host image of the segment table: pointers of parameters and state and the sizes never change
        seg = np.zeros((len(ps), SEG_WORDS), dtype=np.int64)
        seg[:, 0] = [p.data_ptr() for p in ps]
        seg[:, 2] = self._flat1.data_ptr() + 4 * offs[:-1]
        if self._flat2 is not None:
            seg[:, 3] = self._flat2.data_ptr() + 4 * offs[:-1]
        seg[:, 4] = sizes
        self._seg = seg
        self._staging = L.PinnedStaging(torch.int64, min_elems=512)
        self._ready = True

    def add_param_group(self, param_group):
        if self._ready:
            raise PccError("FusedOptimizer: the parameter list is fixed at construction (tables and state buffers are built once)")
        super().add_param_group(param_group)

    # ---- state under torch's names ---------------------------------------------------------------------------------
    def _views(self, i):
        a, n, shape = int(self._offsets[i]), self._params[i].numel(), self._params[i].shape
        st = {}
        if self.mode == "adam":
            st["step"] = self._steps[i]
            st["exp_avg"] = self._flat1[a:a + n].view(shape)
            st["exp_avg_sq"] = self._flat2[a:a + n].view(shape)
        else:
            st["momentum_buffer"] = self._flat1[a:a + n].view(shape)
        return st

    def state_dict(self):
        """Layout of `torch.optim.Adam` / `SGD`; the state tensors are copies, not views into the flat buffers."""
        sd = super().state_dict()
        sd["state"] = {k: {name: (v.clone() if torch.is_tensor(v) else v) for name, v in st.items()} for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """A state dict of this class, of `torch.optim.Adam` (mode 'adam') or of `torch.optim.SGD` (mode 'sgd')."""
        want = ("exp_avg", "exp_avg_sq") if self.mode == "adam" else ("momentum_buffer",)
        for k, st in state_dict["state"].items():
            if st and any(st.get(name) is None for name in want):
                raise PccError(f"load_state_dict: state of parameter {k} lacks {want}: not a state dict of "
                               f"{'Adam' if self.mode == 'adam' else 'SGD with momentum'}")
        super().load_state_dict(state_dict)
        self._flat1.zero_()
        self._steps.zero_()
        if self._flat2 is not None:
            self._flat2.zero_()
        for i, p in enumerate(self._params):
            st = self.state.get(p)
            if not st:
                self.state.pop(p, None)
                continue
            views = self._views(i)
            for name in want:
                views[name].copy_(st[name].to(torch.float32).reshape(p.shape))
            if self.mode == "adam":
                views["step"].fill_(float(st["step"]))
            else:
                self._steps_np[i] = 1.0                   # a momentum buffer exists: the next step is not the first
            self.state[p] = views

    # ---- the step -------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        h = self._staging.acquire(self._seg.size)
        seg = h.numpy().reshape(self._seg.shape)
        seg[:] = self._seg
        stepped = []
        for i, p in enumerate(self._params):
            g = p.grad
            if g is None:
                continue
            if g.is_sparse or g.dtype != torch.float32 or g.device != self.device or not g.is_contiguous() or g.numel() != p.numel():
                raise PccError(f"FusedOptimizer: gradient of parameter {i} must be a dense contiguous float32 tensor on {self.device}")
            if p.data_ptr() != self._seg[i, 0]:
                raise PccError(f"FusedOptimizer: parameter {i} was moved after the optimiser was built (build it after .to(device))")
            seg[i, 1] = g.data_ptr()
            stepped.append(i)
        if not stepped:
            return loss
        self._steps_np[stepped] += 1.0
        seg[:, 5] = self._steps_np
        for i in stepped:
            p = self._params[i]
            if p not in self.state or not self.state[p]:
                self.state[p] = self._views(i)
        with torch.cuda.device(self.device):
            d_seg = self._staging.upload(h, self.device)
            st, ns, nc = L.stream(), len(self._params), self._n_chunks
            clip = self.max_norm is not None
            if clip:
                L.call("pcc_optim_sqnorm", d_seg.data_ptr(), ns, L.ptr(self._chunks), nc, L.ptr(self._partials), self._ws_bytes, st)
            if self.mode == "adam":
                b1, b2 = group["betas"]
                mode = ADAM
            else:
                b1, b2, mode = group["momentum"], 0.0, SGD
            L.call("pcc_optim_step", d_seg.data_ptr(), ns, L.ptr(self._chunks), nc, L.ptr(self._partials), self._ws_bytes, mode,
                   float(group["lr"]), float(b1), float(b2), float(group.get("eps", 0.0)), self.max_norm if clip else 0.0,
                   L.ptr(self.last_norm) if clip else None, st)
        # the kernel wrote the parameters behind autograd's back: packed-weight caches are keyed on (data_ptr, _version)
        torch.autograd.graph.increment_version([self._params[i] for i in stepped])
        return loss
