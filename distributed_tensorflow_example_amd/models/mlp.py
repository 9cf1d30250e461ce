"""The reference's headline model: 784-100-10 MLP trained with SGD
(example.py:69-128; sigmoid hidden layer, softmax output, mean cross-entropy,
GradientDescentOptimizer(0.0005), batch 100 per worker).

* `reference_step`   -- plain PyTorch fp32 (the numerics oracle for the HIP
                        kernels, and the CPU/gloo path of BASELINE config #1).
* `MLP` (nn.Module)  -- generic path built from the framework ops
                        (`ops.linear_act`, `ops.softmax_xent`), used by the
                        TF-compat session layer and autograd users.
* `MLPTrainer`       -- one rank's device state (fp32 master, lr, metrics ring,
                        global step) and its two step engines:
                        `FusedMLPTrainer` (csrc/kernels/mlp_step.hip, 3 launches
                        per step, batch ~100) and `GemmMLPTrainer`
                        (csrc/kernels/mlp_gemm.hip, large batch).
* `MLPStepRunner`    -- replays either trainer's step from hipGraphs over a
                        pinned-host epoch; `PersistentMLPRunner` -- the
                        headline: one persistent launch per chunk of steps
                        (csrc/kernels/mlp_persist_f32.hip).  What they launch
                        next is planned in `mlp_plan.py`.
* `evaluate`         -- held-out loss / accuracy (example.py:187), forward only
                        (csrc/kernels/mlp_eval.hip); also `MLPTrainer.evaluate`
                        on the trainer's own master.  CPU parameters: PyTorch.

Parameter layout (flat fp32, TF variable order and names):
  weights/Variable [784,100], weights/Variable_1 [100,10],
  biases/Variable [100], biases/Variable_1 [10].
"""
from __future__ import annotations

import os
from collections import OrderedDict
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .. import _native
from .mlp_plan import StagePlanner, chunks

D_IN, HIDDEN, N_CLS = 784, 100, 10
OFF_W1, OFF_W2, OFF_B1, OFF_B2 = 0, 78400, 79400, 79500
NPARAM = 79510
PARAM_SPECS: "OrderedDict[str, Tuple[int, Tuple[int, ...]]]" = OrderedDict([
    ("weights/Variable", (OFF_W1, (D_IN, HIDDEN))),
    ("weights/Variable_1", (OFF_W2, (HIDDEN, N_CLS))),
    ("biases/Variable", (OFF_B1, (HIDDEN,))),
    ("biases/Variable_1", (OFF_B2, (N_CLS,))),
])
ACTS = {"sigmoid": 0, "relu": 1}


def init_params(seed: int = 1) -> torch.Tensor:
    """W ~ N(0,1) (tf.random_normal, example.py:84-85), b = 0 (example.py:89-90)."""
    g = torch.Generator().manual_seed(seed)
    p = torch.zeros(NPARAM, dtype=torch.float32)
    p[OFF_W1:OFF_W2] = torch.randn(D_IN * HIDDEN, generator=g)
    p[OFF_W2:OFF_B1] = torch.randn(HIDDEN * N_CLS, generator=g)
    return p


def unflatten(flat: torch.Tensor) -> Dict[str, torch.Tensor]:
    out = {}
    for name, (off, shape) in PARAM_SPECS.items():
        n = int(np.prod(shape))
        out[name] = flat[off:off + n].view(*shape)
    return out


def _act(z, act):
    return torch.sigmoid(z) if act == "sigmoid" else torch.relu(z)


def reference_forward(flat: torch.Tensor, x: torch.Tensor, act: str = "sigmoid"):
    p = unflatten(flat)
    z2 = x @ p["weights/Variable"] + p["biases/Variable"]
    a2 = _act(z2, act)
    z3 = a2 @ p["weights/Variable_1"] + p["biases/Variable_1"]
    return z3


def reference_loss_and_grad(flat: torch.Tensor, x: torch.Tensor, labels: torch.Tensor,
                            act: str = "sigmoid", naive: bool = False):
    """fp32 loss, accuracy and flat gradient (autograd) of one batch."""
    w = flat.detach().clone().requires_grad_(True)
    z3 = reference_forward(w, x.float(), act)
    y = torch.nn.functional.one_hot(labels.long(), N_CLS).float()
    if naive:  # -sum(y * log(softmax)) exactly as example.py:103 (can be inf/NaN)
        loss = torch.mean(-torch.sum(y * torch.log(torch.softmax(z3, 1)), 1))
    else:
        loss = torch.nn.functional.cross_entropy(z3, labels.long())
    loss.backward()
    acc = (z3.argmax(1) == labels.long()).float().mean()
    return loss.detach(), acc.detach(), w.grad.detach()


def reference_step(flat: torch.Tensor, x: torch.Tensor, labels: torch.Tensor, lr: float,
                   act: str = "sigmoid"):
    loss, acc, g = reference_loss_and_grad(flat, x, labels, act)
    flat.sub_(lr * g)
    return loss, acc


def _eval_params(params):
    """(W1, b1, W2, b2) of a flat tensor in this module's layout or of the four tensors."""
    if isinstance(params, torch.Tensor):
        if params.dim() != 1 or params.numel() != NPARAM:
            raise ValueError(f"flat parameters must have {NPARAM} elements")
        p = unflatten(params.detach())
        return (p["weights/Variable"], p["biases/Variable"], p["weights/Variable_1"], p["biases/Variable_1"])
    W1, b1, W2, b2 = (t.detach() for t in params)
    return W1, b1, W2, b2


def _eval_labels(labels):
    """Labels as the kernel takes them: uint8 / int32 ids [N] or a float32 one-hot [N, C]."""
    if isinstance(labels, torch.Tensor):
        if labels.dim() == 2 and labels.dtype == torch.float32:
            return labels
        if labels.dim() != 1 or labels.is_floating_point():
            raise ValueError("labels must be integer class ids [N] or a float32 one-hot [N, C]")
        return labels if labels.dtype in (torch.uint8, torch.int32) else labels.to(torch.int32)
    labels = np.asarray(labels)
    if labels.ndim == 2 and labels.dtype == np.float32:
        return labels
    if labels.ndim != 1 or labels.dtype.kind not in "iu":
        raise ValueError("labels must be integer class ids [N] or a float32 one-hot [N, C]")
    return labels if labels.dtype in (np.uint8, np.int32) else labels.astype(np.int32)


def _evaluate_cpu(W1, b1, W2, b2, x, labels, act, naive, return_predictions):
    """The same quantities with PyTorch fp32 on the host (gloo / CPU path)."""
    x = torch.as_tensor(x)
    labels = torch.as_tensor(labels)
    xf = x.to(torch.float32) / 255.0 if x.dtype == torch.uint8 else x.to(torch.float32)
    z3 = _act(xf @ W1 + b1, act) @ W2 + b2
    y = labels if labels.dim() == 2 else torch.nn.functional.one_hot(labels.long(), W2.shape[1]).float()
    ids = labels.argmax(1) if labels.dim() == 2 else labels.long()
    if naive:
        rows = -torch.sum(y * torch.log(torch.softmax(z3, 1)), 1)
    else:
        rows = -torch.sum(y * torch.log_softmax(z3, 1), 1)
    pred = z3.argmax(1)
    loss = float(rows.double().sum()) / x.shape[0]
    acc = int((pred == ids).sum()) / x.shape[0]
    return (loss, acc, pred.to(torch.int32)) if return_predictions else (loss, acc)


def _host_tensor(a: np.ndarray) -> torch.Tensor:
    """A tensor view of a host array that is only read (a read-only array is fine)."""
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return torch.from_numpy(a)


_EVAL_STAGE = {}     # device -> two device staging slots (grown on demand), their events, the side stream


def _eval_stage(dev, xbytes, lbytes):
    st = _EVAL_STAGE.get(dev)
    if st is None or st["xcap"] < xbytes or st["lcap"] < lbytes:
        xcap = max(xbytes, st["xcap"] if st else 0)
        lcap = max(lbytes, st["lcap"] if st else 0)
        st = _EVAL_STAGE[dev] = dict(
            xcap=xcap, lcap=lcap,
            dx=[torch.empty(xcap, dtype=torch.uint8, device=dev) for _ in range(2)],
            dl=[torch.empty(lcap, dtype=torch.uint8, device=dev) for _ in range(2)],
            used=[None, None], side=st["side"] if st else torch.cuda.Stream(device=dev))
    return st


def evaluate(params, x, labels, act: str = "sigmoid", naive: bool = False, chunk_rows: int = 16384,
             return_predictions: bool = False):
    """Mean loss and accuracy of the model on held-out rows, forward only
    (example.py:187).  Returns `(loss, accuracy)` as Python floats, and the int32
    predictions (argmax of the logits, first maximum on ties) as well with
    `return_predictions`.

    params: the flat tensor of this module's layout, or the four tensors
        (W1 [K, H], b1 [H], W2 [H, C], b2 [C]).
    x: [N, K] uint8 pixels (evaluated as x / 255, bit-identical to the loader's
        float32 array) or float32; a device tensor or a NumPy array.
    labels: class ids [N] or a float32 one-hot [N, C]; device tensor or NumPy.
    naive: the loss as -sum(y_ log softmax) (example.py:103), else the stable form.

    GPU parameters run csrc/kernels/mlp_eval.hip on the current stream, behind
    the work already queued there.  Host arrays go to two device staging
    buffers on a side stream, `chunk_rows` rows at a time, so device memory
    stays bounded for any N: the copy of chunk i + 1 overlaps the kernel of
    chunk i (events order the two streams), the kernel accumulates into a
    device record and ONE device-to-host copy fetches it at the end.  The
    copies read the caller's arrays in place: a pinned staging copy in front of
    them cost more than it saved (10,000 x 784 float32: 1.3-1.4 ms against
    0.74-0.83 ms, the single-threaded host copy being slower than the
    transfer; profiles/mlp_eval_ab.json).  CPU parameters compute the same
    quantities with PyTorch."""
    W1, b1, W2, b2 = _eval_params(params)
    if x.ndim != 2:
        raise ValueError("x must be [N, K]")
    N, K = int(x.shape[0]), int(x.shape[1])
    if N == 0:
        raise ValueError("evaluate needs at least one row")
    labels = _eval_labels(labels)
    if labels.shape[0] != N:
        raise ValueError("x and labels differ in rows")
    if not W1.is_cuda:
        return _evaluate_cpu(W1, b1, W2, b2, x, labels, act, naive, return_predictions)
    C_ = _native.load()
    dev = W1.device
    args = (W1.contiguous(), b1.contiguous(), W2.contiguous(), b2.contiguous(), ACTS[act], bool(naive))
    with torch.cuda.device(dev):
        rec = torch.empty(3, dtype=torch.int64, device=dev)
        pred = torch.empty(N, dtype=torch.int32, device=dev) if return_predictions else None
        x_host, l_host = not isinstance(x, torch.Tensor), not isinstance(labels, torch.Tensor)
        if x_host:
            x = np.ascontiguousarray(x if x.dtype in (np.uint8, np.float32) else x.astype(np.float32))
        elif x.dtype not in (torch.uint8, torch.float32):
            x = x.float()
        if l_host:
            labels = np.ascontiguousarray(labels)
        if not (x_host and l_host):
            xd = torch.tensor(x, device=dev) if x_host else x.to(dev).contiguous()
            ld = torch.tensor(labels, device=dev) if l_host else labels.to(dev).contiguous()
            C_.mlp_eval(xd, ld, *args, rec, True, pred, None)
        else:
            R = min(int(chunk_rows), N)
            if R < 1:
                raise ValueError("chunk_rows must be positive")
            xrow, lrow = K * x.itemsize, labels[0].size * labels.itemsize    # bytes per row (C-contiguous)
            st = _eval_stage(dev, R * xrow, R * lrow)
            main, side = torch.cuda.current_stream(), st["side"]
            side.wait_stream(main)      # (a freshly allocated slot may be memory the queued work still uses)
            xdt = torch.uint8 if x.dtype == np.uint8 else torch.float32
            ldt = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32,
                   np.dtype(np.float32): torch.float32}[labels.dtype]
            xb = _host_tensor(np.asarray(x).reshape(-1).view(np.uint8))
            lb = _host_tensor(np.asarray(labels).reshape(-1).view(np.uint8))
            for i, r0 in enumerate(range(0, N, R)):
                n = min(R, N - r0)
                s = i % 2
                with torch.cuda.stream(side):
                    if st["used"][s] is not None:
                        side.wait_event(st["used"][s])      # the kernel that last read this device slot is done
                    st["dx"][s][:n * xrow].copy_(xb[r0 * xrow:(r0 + n) * xrow], non_blocking=True)
                    st["dl"][s][:n * lrow].copy_(lb[r0 * lrow:(r0 + n) * lrow], non_blocking=True)
                    copied = torch.cuda.Event()
                    copied.record(side)
                main.wait_event(copied)
                xd = st["dx"][s][:n * xrow].view(xdt).view(n, K)
                ld = st["dl"][s][:n * lrow].view(ldt).view((n,) + tuple(labels.shape[1:]))
                C_.mlp_eval(xd, ld, *args, rec, i == 0, None if pred is None else pred[r0:r0 + n], None)
                st["used"][s] = torch.cuda.Event()
                st["used"][s].record(main)
        r = rec.cpu()                                    # the one read-back: {loss sum (fp64), correct, rows}
    loss = float(r.view(torch.float64)[0]) / int(r[2])
    acc = int(r[1]) / int(r[2])
    return (loss, acc, pred) if return_predictions else (loss, acc)


class MLP(torch.nn.Module):
    """Generic-path MLP on the framework's fused ops (autograd-enabled)."""

    def __init__(self, act: str = "sigmoid", seed: int = 1, device=None):
        super().__init__()
        flat = init_params(seed)
        p = unflatten(flat)
        self.W1 = torch.nn.Parameter(p["weights/Variable"].clone())
        self.W2 = torch.nn.Parameter(p["weights/Variable_1"].clone())
        self.b1 = torch.nn.Parameter(p["biases/Variable"].clone())
        self.b2 = torch.nn.Parameter(p["biases/Variable_1"].clone())
        self.act = act
        if device is not None:
            self.to(device)

    def tf_variables(self) -> "OrderedDict[str, torch.nn.Parameter]":
        return OrderedDict([("weights/Variable", self.W1), ("weights/Variable_1", self.W2),
                            ("biases/Variable", self.b1), ("biases/Variable_1", self.b2)])

    def forward(self, x):
        from ..ops import linear_act

        a2 = linear_act(x, self.W1, self.b1, self.act)
        return linear_act(a2, self.W2, self.b2, "none")


class MLPTrainer:
    """One rank's training state on the device: the flat fp32 master, the
    learning rate, the (loss, accuracy) ring and the global step.  An engine adds
    its scratch buffers, `refresh_shadows` (whatever it derives from the master),
    `enqueue_step` and `step_tensors`, and ends its constructor with `set_params`."""

    def __init__(self, batch_size: int, lr: float, act: str, world, naive_loss: bool, metrics_ring: int, device):
        self.C = _native.load()
        self.world = world
        self.world_size = 1 if world is None else world.world_size
        self.device = dev = device or torch.device("cuda", torch.cuda.current_device())
        self.B = int(batch_size)
        self.act = ACTS[act]
        self.act_name = act
        self.naive = bool(naive_loss)
        self.params = torch.zeros(NPARAM, dtype=torch.float32, device=dev)
        self.lr = torch.tensor([lr], dtype=torch.float32, device=dev)
        self.ring = int(metrics_ring)
        self.metrics = torch.zeros(self.ring * 2, dtype=torch.float32, device=dev)
        self.gstep = torch.zeros(1, dtype=torch.int64, device=dev)
        self.allreduce = "none"
        self.ipc_parity = 0          # exchange slot of the next step (`MLPStepRunner` plans it per graph)
        self.shadows_stale = False   # set by PersistentMLPRunner (it updates only the fp32 master)

    def ipc_error(self) -> int:
        return 0

    def set_params(self, flat_cpu: torch.Tensor, broadcast: bool = True):
        self.params.copy_(flat_cpu.to(self.device, torch.float32))
        if broadcast and self.world is not None and self.world_size > 1:
            self.world.broadcast(self.params, 0)  # chief init + broadcast
        self.refresh_shadows()

    def get_params(self) -> torch.Tensor:
        return self.params.detach().cpu()

    def set_lr(self, lr: float):
        self.lr.fill_(lr)

    @property
    def global_step(self) -> int:
        return int(self.gstep.item())

    def set_global_step(self, v: int):
        self.gstep.fill_(int(v))

    def read_metrics(self, first_step: int, last_step: int) -> np.ndarray:
        """(loss, accuracy) rows for global steps [first, last)."""
        m = self.metrics.view(self.ring, 2).cpu().numpy()
        return m[np.arange(first_step, last_step) % self.ring]

    def evaluate(self, x, labels, **kw):
        """`evaluate` on this trainer's fp32 master with its activation and loss
        form, on the current stream behind the steps already queued (a call after
        `PersistentMLPRunner.run` sees the trained parameters).  Changes nothing:
        parameters, global_step and the metrics ring stay as they are."""
        return evaluate(self.params, x, labels, act=self.act_name, naive=self.naive, **kw)


class FusedMLPTrainer(MLPTrainer):
    """The small-batch step (csrc/kernels/mlp_step.hip): 3 launches on 1 GPU
    (`mlp_l1_fwd`, `mlp_head_bwd`, `mlp_wgrad` with SGD in its epilogue); in sync
    data parallel the gradient exchange inside `mlp_wgrad` over IPC ("ipc-fused"),
    after it over IPC ("ipc-apply") or RCCL, or left to the caller ("external")."""

    def __init__(self, batch_size: int = 100, lr: float = 0.0005, act: str = "sigmoid",
                 world=None, grad_dtype: torch.dtype = torch.bfloat16, naive_loss: bool = False,
                 metrics_ring: int = 8192, seed: int = 1, device=None, allreduce: str = "auto",
                 ipc_timeout_s: float = 5.0):
        super().__init__(batch_size, lr, act, world, naive_loss, metrics_ring, device)
        dev, B, bf = self.device, self.B, torch.bfloat16
        self.nb = (B + 15) // 16
        self.W1T = torch.zeros(112 * 800, dtype=bf, device=dev)
        self.W2T = torch.zeros(16 * 128, dtype=bf, device=dev)
        self.W2N = torch.zeros(112 * 32, dtype=bf, device=dev)
        self.z2p = torch.zeros(self.C.mlp_ksplit() * self.nb * 16 * 112, dtype=torch.float32,
                               device=dev)
        self.dz2T = torch.zeros(112 * ((B + 31) // 32) * 32, dtype=bf, device=dev)
        self.partials = torch.zeros(self.nb * 1112, dtype=torch.float32, device=dev)
        self.grad_dtype = grad_dtype
        self.grads = (torch.zeros(NPARAM, dtype=grad_dtype, device=dev)
                      if self.world_size > 1 else None)
        self.ipc = None
        self.ipc_mode = None
        self.ipc_timeout_s = float(ipc_timeout_s)
        if self.world_size > 1 and allreduce == "external":
            # the caller owns the gradient exchange (PersistentMLPRunner: in-kernel
            # over IPC): no exchange buffers, no RCCL communicator
            self.allreduce = "external"
        elif self.world_size > 1:
            self.allreduce = "rccl"
            if allreduce in ("ipc", "ipc-fused", "ipc-apply", "auto"):
                try:
                    self._setup_ipc()
                    self.ipc_mode = "apply" if allreduce == "ipc-apply" else "fused"
                    self.allreduce = "ipc-" + self.ipc_mode
                except Exception as e:  # noqa: BLE001
                    if allreduce.startswith("ipc"):
                        raise
                    import warnings

                    warnings.warn(f"IPC all-reduce unavailable ({e}); using RCCL")
            if self.allreduce == "rccl":
                # created here, collectively, only when this trainer's exchange is RCCL
                # (RuntimeError if it cannot come up: the caller falls back)
                world.ensure_comm()
        # RCCL and the IPC kernels capture into hipGraphs; a gloo all-reduce (ranks
        # sharing one GPU in tests) does not
        self.graph_safe = (self.world_size == 1 or self.allreduce.startswith("ipc")
                           or (world is not None and world.comm is not None))
        self.set_params(init_params(seed))

    # ---------------------------------------------------------------- IPC one-shot all-reduce
    def _setup_ipc(self):
        """Map every rank's gradient buffer (xGMI peers of one node); handles go
        through the gloo control plane.  Layout: [flags][grad slot 0][grad slot 1]."""
        w = self.world
        if int(os.environ.get("LOCAL_WORLD_SIZE", w.world_size)) != w.world_size:
            raise RuntimeError("IPC all-reduce needs all ranks on one node")
        C = self.C
        self.ipc_flag_bytes = C.mlp_ipc_flag_bytes()
        self.ipc_slot = ((NPARAM * 2 + 255) // 256) * 256
        from ..parallel.world import open_peer_buffers
        buf = open_peer_buffers(C, self.ipc_flag_bytes + 2 * self.ipc_slot, w)
        self.ipc = buf
        self.ipc_grads = [buf.tensor(self.ipc_flag_bytes + p * self.ipc_slot, NPARAM, 1) for p in (0, 1)]
        self.ipc_err = torch.zeros(1, dtype=torch.int32, device=self.device)

    def ipc_error(self) -> int:
        return int(self.ipc_err.item()) if self.ipc is not None else 0

    def refresh_shadows(self):
        self.C.mlp_apply_flat(self.params, None, self.lr, 0.0, self.W1T, self.W2T, self.W2N)
        self.shadows_stale = False

    # ----------------------------------------------------------------- steps
    def enqueue_step(self, x: torch.Tensor, x_off: int, x_kind: int, labels: torch.Tensor,
                     labels_off: int, ipc_parity: Optional[int] = None):
        """Enqueue one full training step on the current stream.

        x: device buffer holding B rows of 784 features at byte offset x_off
        (kind 0 uint8 pixels, 1 fp32, 2 bf16); labels: uint8 class ids.
        """
        C, B = self.C, self.B
        if self.shadows_stale:
            self.refresh_shadows()
        C.mlp_l1_fwd(x, x_off, x_kind, B, self.W1T, self.z2p)
        C.mlp_head_bwd(self.z2p, labels, labels_off, B, self.W2T, self.W2N, self.params, self.dz2T,
                       self.partials, 1.0 / B, self.act, self.naive, self.gstep)

        def wgrad(grads, grad_kind, *ipc_tail):
            C.mlp_wgrad(x, x_off, x_kind, self.dz2T, B, self.partials, self.params, self.W1T, self.W2T, self.W2N,
                        grads, grad_kind, self.lr, self.metrics, self.gstep, *ipc_tail)

        if self.world_size == 1:
            wgrad(None, 0)
        elif self.ipc is not None:
            par = self.ipc_parity if ipc_parity is None else int(ipc_parity) & 1
            if ipc_parity is None:
                self.ipc_parity ^= 1
            if self.ipc_mode == "fused":
                # every wgrad workgroup swaps its gradient block with the same workgroup
                # on all peers (IPC over xGMI) and applies SGD in place: 3 launches/step
                wgrad(None, 3, None, self.ipc.table_ptr(), self.world_size, self.world.rank, par, self.ipc_slot,
                      self.ipc_err, self.ipc_timeout_s)
            else:
                # one-shot: bf16 grads into this rank's exported slot, then every rank
                # sums all peers' slots over xGMI inside the SGD apply kernel
                wgrad(self.ipc_grads[par], 2)
                C.mlp_ipc_reduce_apply(self.params, self.ipc.table_ptr(), self.world_size, self.world.rank, par,
                                       self.ipc_slot, self.gstep, self.lr, 1.0 / self.world_size, self.W1T,
                                       self.W2T, self.W2N, self.ipc_err, self.ipc_timeout_s)
        else:
            wgrad(self.grads, 1 if self.grad_dtype == torch.float32 else 2)
            self.world.all_reduce(self.grads, "sum")
            C.mlp_apply_flat(self.params, self.grads, self.lr, 1.0 / self.world_size, self.W1T,
                             self.W2T, self.W2N)

    def step_tensors(self, x: torch.Tensor, labels: torch.Tensor):
        """Eager step on device tensors (x: uint8/fp32/bf16 [B,784], labels [B])."""
        kind = {torch.uint8: 0, torch.float32: 1, torch.bfloat16: 2}[x.dtype]
        self.enqueue_step(x.contiguous(), 0, kind, labels.to(torch.uint8).contiguous(), 0)


class GemmMLPTrainer(MLPTrainer):
    """Large-batch step of the same model (csrc/kernels/mlp_gemm.hip), 4
    launches: `mlpg_l1` (one workgroup per 64 rows x 16 hidden units: the
    hidden layer on bf16 MFMA with W1 as an exact 3-way bf16 split) and
    `mlpg_head` (one workgroup per 16 rows, its waves splitting the hidden
    tiles: logits, softmax-xent, dz2 and the dW2/db2 partials on exact-f32 MFMA),
    `mlpg_wgrad` ([dW1; db1] over a 64-pixel-block x 256-row-chunk grid, dz2 as
    its exact split) and `mlpg_apply` (fixed-order slab reduction, SGD, W1
    fragment-image refresh, metrics).  The fused engines contract the batch serially inside
    one wave per weight tile: right at B=100, 4x too slow at B=4096.  All three
    launches are graph-capturable, so `MLPStepRunner` replays them exactly like
    the fused trainer's.  N > 1: the apply kernel first writes the reduced flat
    fp32 gradient, one RCCL all-reduce, then the apply."""

    def __init__(self, batch_size: int = 4096, lr: float = 0.0005, act: str = "sigmoid", world=None,
                 naive_loss: bool = False, metrics_ring: int = 8192, seed: int = 1, device=None,
                 **_ignored):
        super().__init__(batch_size, lr, act, world, naive_loss, metrics_ring, device)
        dev, B, f32 = self.device, self.B, torch.float32
        BP = (B + 63) // 64 * 64
        # dW1: one workgroup per (64-pixel block, 128- or 256-row batch chunk); the
        # B-fragment image of dz2 is padded (with zeros) to whole chunks
        wc = self.C.mlpg_wchunk(B)
        self.nchunk = (B + wc - 1) // wc
        self.W1S = torch.zeros(3 * 112 * 800, dtype=torch.bfloat16, device=dev)
        self.dz2S = torch.zeros(3 * 112 * self.nchunk * wc, dtype=torch.bfloat16, device=dev)
        self.a2 = torch.zeros(BP * 112, dtype=f32, device=dev)
        self.P1 = torch.zeros(BP // 16 * self.C.mlpg_p1_floats(), dtype=f32, device=dev)
        self.P2 = torch.zeros(self.nchunk * self.C.mlpg_p2_floats(), dtype=f32, device=dev)
        self.grads = torch.zeros(NPARAM, dtype=f32, device=dev) if self.world_size > 1 else None
        if self.world_size > 1:
            coll = world.gpu_coll(NPARAM * 4)    # collective: IPC on one node, else RCCL; None on gloo worlds
            self.allreduce = "ipc" if (coll is not None and coll is world.ipc) else \
                ("rccl" if world.comm is not None else world.backend)
        # RCCL and the IPC collectives capture into hipGraphs (the IPC sequence
        # numbers live on the device); a gloo all-reduce does not
        self.graph_safe = self.world_size == 1 or self.allreduce in ("rccl", "ipc")
        self.set_params(init_params(seed))

    def _apply(self, mode: int, gin=None, gout=None, scale: float = 1.0):
        self.C.mlpg_apply(self.params, self.P1, self.P2, self.nchunk, gin, gout, self.lr, scale, self.W1S,
                          self.metrics, self.gstep, self.B, mode)

    def refresh_shadows(self):
        self._apply(3)

    def enqueue_step(self, x: torch.Tensor, x_off: int, x_kind: int, labels: torch.Tensor,
                     labels_off: int, ipc_parity: Optional[int] = None):
        """x: u8 stage holding B rows of 784 pixels at byte offset x_off; labels: u8 class ids."""
        if x_kind != 0:
            raise ValueError("GemmMLPTrainer reads uint8 pixel records (x_kind 0)")
        C, B = self.C, self.B
        C.mlpg_fwd(x, x_off, labels, labels_off, B, self.W1S, self.params, self.a2, self.P1, self.dz2S, self.act,
                   self.naive, 1.0 / B)
        C.mlpg_wgrad(x, x_off, B, self.dz2S, self.P2, self.nchunk)
        if self.world_size == 1:
            self._apply(0)
        else:
            self._apply(1, gout=self.grads)
            self.world.all_reduce(self.grads, "sum")
            self._apply(2, gin=self.grads, scale=1.0 / self.world_size)

    def step_tensors(self, x: torch.Tensor, labels: torch.Tensor):
        """Eager step on device tensors (x: uint8 [B,784], labels [B])."""
        if x.dtype != torch.uint8:
            raise ValueError("GemmMLPTrainer.step_tensors takes uint8 pixels")
        self.enqueue_step(x.contiguous().view(-1), 0, 0, labels.to(torch.uint8).contiguous(), 0)


class MLPStepRunner:
    """Drives either trainer's `enqueue_step` over a pinned-host epoch.

    The epoch lives batch-major in pinned host memory; the device holds only a
    *chunk* stage of `g` batches (g*78.5 KB at B=100).  Each chunk is one
    hipGraph: hipMemcpyAsync(chunk, pinned -> stage) followed by the `g` fused
    steps; the host issues one launch per `g` steps.

    prefetch="serial" (default): the copy is a node at the head of the chunk
        graph on the compute stream (+1.7 us/step amortised: 85 us per 3.9 MB
        chunk at PCIe rate).
    prefetch="side": double-buffered stage, the next chunk is copied on a side
        stream under the current replay, synchronised by events.  On MI355X /
        ROCm 7 every cross-queue event dependency costs ~150 us of GPU idle
        (measured, scripts/probes/diag_mlp3.py: 14.9 us/step vs 13.2 serial; the same
        fork/join captured inside the graph: 16.4), so it only pays where
        cross-queue waits are cheap.
    """

    def __init__(self, trainer: MLPTrainer, epoch, steps_per_graph: int = 50,
                 use_graph: bool = True, prefetch: str = "serial"):
        if prefetch not in ("serial", "side"):
            raise ValueError("prefetch must be 'serial' or 'side'")
        self.t = trainer
        self.epoch = epoch
        # a chunk may run across the epoch boundary (its records are copied in two
        # pieces): at large batch an epoch is only ~13 steps, and the side-stream
        # prefetch pays its cross-queue synchronisation once per chunk
        self.g = int(max(1, steps_per_graph))
        self.use_graph = use_graph
        self.prefetch = prefetch
        self.side = None       # (side) the copy stream, made by the first run()
        self.graphs: Dict[tuple, torch.cuda.CUDAGraph] = {}
        nbuf = 2 if prefetch == "side" else 1
        self.stage = [torch.zeros(self.g * epoch.rec, dtype=torch.uint8, device=trainer.device)
                      for _ in range(nbuf)]
        self.cursor = 0        # next batch index (global)
        self.parity = 0        # (side) stage buffer holding the chunk at `cursor`
        self.loaded = None     # (side) (b0, g) resident in stage[parity]
        self._freed = None     # (side) event: last replay reading stage[parity ^ 1] done

    def _copy_chunk(self, dst: torch.Tensor, b0: int, g: int):
        ep = self.epoch
        nb, off = ep.num_batches, 0
        while g > 0:   # batches b0 .. b0+g-1 of the epoch, wrapping at its end
            n = min(g, nb - b0)
            self.t.C.memcpy_h2d_async(dst, off, ep.host, b0 * ep.rec, n * ep.rec)
            off += n * ep.rec
            b0 = (b0 + n) % nb
            g -= n

    def _emit_steps(self, g: int, buf: torch.Tensor, ipar: int):
        t = self.t
        rec, B = self.epoch.rec, t.B
        for i in range(g):
            off = i * rec
            t.enqueue_step(buf, off, 0, buf, off + B * D_IN, ipc_parity=(ipar + i) & 1)

    def _emit(self, key):
        if self.prefetch == "serial":
            b0, g, ipar = key
            self._copy_chunk(self.stage[0], b0, g)
            self._emit_steps(g, self.stage[0], ipar)
        else:
            g, par, ipar = key
            self._emit_steps(g, self.stage[par], ipar)

    def _graph(self, key) -> torch.cuda.CUDAGraph:
        gr = self.graphs.get(key)
        if gr is None:
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            s = torch.cuda.Stream(device=self.t.device)
            with torch.cuda.graph(gr, stream=s):
                self._emit(key)
            torch.cuda.synchronize()
            self.graphs[key] = gr
        return gr

    def plan(self, steps: int):
        """[(b0, g, parity, next, ipc_parity)] for the next `steps` steps from the cursor."""
        nb = self.epoch.num_batches
        ch = chunks(self.cursor, steps, self.g, nb, wrap=True)
        after = chunks(self.cursor + steps, self.g, self.g, nb, wrap=True)[0]  # speculative prefetch
        out, par, ipar = [], self.parity, self.t.ipc_parity
        for j, (b0, g) in enumerate(ch):
            nxt = ch[j + 1] if j + 1 < len(ch) else after
            out.append((b0, g, par, nxt, ipar))
            par ^= 1
            ipar = (ipar + g) & 1
        return out

    def _key(self, b0, g, par, ipar=0):
        return (b0, g, ipar) if self.prefetch == "serial" else (g, par, ipar)

    def prepare(self, steps: int):
        """Capture every graph `run(steps)` will need (keeps capture out of timing)."""
        if self.use_graph:
            for (b0, g, par, _, ipar) in self.plan(steps):
                self._graph(self._key(b0, g, par, ipar))

    def run(self, steps: int, events: Optional[list] = None):
        main = torch.cuda.current_stream()
        if self.prefetch == "side" and self.side is None:
            self.side = torch.cuda.Stream(device=self.t.device)
        for (b0, g, par, nxt, ipar) in self.plan(steps):
            key = self._key(b0, g, par, ipar)
            self.t.ipc_parity = (ipar + g) & 1
            if self.prefetch == "side" and self.loaded != (b0, g):  # cold start / plan change
                self._copy_chunk(self.stage[par], b0, g)
                self._freed = None
            if self.use_graph:
                self._graph(key).replay()
            else:
                self._emit(key)
            if events is not None:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record(main)
                events.append((ev, g))
            if self.prefetch == "side":
                # next chunk into the other buffer, behind the end of the replay that
                # last read it; fresh events (no re-record with pending waits)
                ev_copy = torch.cuda.Event()
                if self._freed is not None:
                    self.side.wait_event(self._freed)
                with torch.cuda.stream(self.side):
                    self._copy_chunk(self.stage[par ^ 1], nxt[0], nxt[1])
                ev_copy.record(self.side)
                self._freed = torch.cuda.Event()
                self._freed.record(main)
                main.wait_event(ev_copy)
                self.parity = par ^ 1
                self.loaded = nxt
            self.cursor += g


class PersistentMLPRunner:
    """Drives a persistent weight-stationary training kernel over a pinned-host
    epoch: ONE launch per chunk of up to `g` steps.

    precision="fp32" (default, the reference's precision: example.py:77-118 is
        fp32 end to end) -- csrc/kernels/mlp_persist_f32.hip, SPLIT: 28 compute
        workgroups (7 hidden blocks x 4 feature slices, packed on one XCD); the
        two big GEMMs (x W1 and x^T dz2) on 16x16x32 bf16 MFMA through the EXACT
        3-way split of their fp32 operand (hi + mid + lo == the fp32 value;
        pixels exact in bf16), so every product is exact and accumulates in
        fp32; the head on f32-input MFMA; fp32 master weights in VGPRs.  Each
        step's x slice is staged into LDS by one wave with LDS-DMA.
    precision="fp32-mfma" -- the same engine with every product on f32-input
        MFMA (v_mfma_f32_16x16x4_f32, bitwise an fmaf chain): 1/8 of the bf16
        MFMA rate, ~2 us/step slower.
    (Rounds 1-3 also carried a 7-workgroup split engine -- one hand-off per
    step but 7 CUs of MFMA work: 14.5 us/step -- and an fp16 engine; both were
    retired in round 4: profiles/README.md.)

    Inside each launch the copier workgroups pull the NEXT chunk from pinned host
    memory over PCIe into the other device stage while the compute workgroups
    run this one.  No second stream, no cross-queue events, no graph capture.

    Which chunk a launch runs and which it copies is `mlp_plan.StagePlanner`'s
    business (`lookahead`: e.g. a warmup priming exactly the timed run); its
    `cursor`, `staged`, `copy_only_launches` and `last_prefetch_steps` read here.

    N GPUs of one node (world_size > 1): every compute workgroup exchanges its
    gradient with the same workgroup on every peer through IPC-mapped uncached
    buffers inside the same launch (flag per workgroup and step, rank-order sums
    -> bit-identical replicas).  Batch <= 112 per GPU.

    `step_ts` (int64 ring on the device) receives the s_memrealtime (100 MHz)
    stamp of every global step's start, plus the end of each launch:
    `step_times_ms(first, last)` gives true per-step durations.
    """

    TS_RING = 16384

    def __init__(self, trainer: FusedMLPTrainer, epoch, steps_per_launch: int = 550,
                 timeout_s: float = 30.0, precision: str = "fp32", grad_bf16: bool = True,
                 placement: str = "auto", exchange: str = "one-shot"):
        C = trainer.C
        if precision not in ("fp32", "fp32-mfma"):
            raise ValueError("precision must be 'fp32' or 'fp32-mfma'")
        self.precision = precision
        if exchange not in ("one-shot", "two-shot"):
            raise ValueError("exchange must be 'one-shot' or 'two-shot'")
        # N GPUs: one-shot = each workgroup reads its gradient slot from every
        # peer ((W-1) slots per GPU per step); two-shot = reduce-scatter by wave
        # chunk + all-gather of the sums (2 (W-1)/W of a slot, one more hop)
        self.exchange = exchange
        maxb = C.mlpf_max_batch()
        if trainer.B > maxb:
            raise ValueError(f"PersistentMLPRunner needs batch <= {maxb}")
        if epoch.batch_size != trainer.B:
            raise ValueError("epoch batch size != trainer batch size")
        self.t = t = trainer
        self.epoch = epoch
        self.g = int(min(steps_per_launch, epoch.num_batches))
        if placement == "auto":
            # several ranks sharing one GPU (tests): their compute workgroups cannot all sit on one XCD
            nloc = int(os.environ.get("LOCAL_WORLD_SIZE", "1"))
            placement = "spread" if nloc > max(1, torch.cuda.device_count()) else "packed"
        if placement not in ("packed", "spread"):
            raise ValueError("placement must be 'auto', 'packed' or 'spread'")
        self.placement = placement
        dev = t.device
        stages = [torch.zeros(self.g * int(C.mlpf_stage_rec()), dtype=torch.uint8, device=dev) for _ in range(2)]
        xbuf = torch.zeros(int(C.mlpf_xbuf_bytes()), dtype=torch.uint8, device=dev)
        seq = torch.zeros(1, dtype=torch.int64, device=dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.step_ts = torch.zeros(self.TS_RING, dtype=torch.int64, device=dev)
        self._phase_ts = None   # optional [64 steps][64 wg][16] phase stamps (profiling): `phase_ts`
        self.use_graph = False  # MLPStepRunner interface
        self.prefetch = "in-kernel"
        self.ipc = None
        W, rank = 1, 0
        w = t.world
        if w is not None and w.world_size > 1:
            if int(os.environ.get("LOCAL_WORLD_SIZE", w.world_size)) != w.world_size:
                raise RuntimeError("the persistent N-GPU exchange needs all ranks on one node")
            from ..parallel.world import open_peer_buffers
            self.ipc = open_peer_buffers(C, int(C.mlpf_ipc_bytes()), w)
            W, rank = w.world_size, w.rank
        # the prepared C++ launcher: every tensor checked and every pointer resolved once (it keeps
        # the stages, xbuf and seq alive), so a launch is a call with 5 ints
        self._plan = C.PersistF32Plan(
            stages[0], stages[1], epoch.rec, t.B, t.params, t.lr, t.metrics, t.gstep, seq, xbuf, self.err,
            float(timeout_s), t.act, int(t.naive), epoch.host, self.step_ts,
            self.ipc.table_ptr() if self.ipc is not None else 0, W, rank, bool(grad_bf16),
            placement == "spread", exchange == "two-shot", precision == "fp32")
        self._stage = StagePlanner(epoch.num_batches, epoch.rec, self.g, self._plan.launch)
        self.prepare = self._stage.prepare          # stage the first chunk of the next run(steps), untimed
        self.invalidate = self._stage.invalidate    # after re-packing the pinned epoch (a shuffle)

    # the staging state lives in the planner (`cursor` and `staged` may be assigned)
    cursor = property(lambda self: self._stage.cursor, lambda self, v: setattr(self._stage, "cursor", v))
    staged = property(lambda self: self._stage.staged, lambda self, v: setattr(self._stage, "staged", v))
    copy_only_launches = property(lambda self: self._stage.copy_only_launches)
    last_prefetch_steps = property(lambda self: self._stage.last_prefetch_steps)

    @property
    def phase_ts(self):
        return self._phase_ts

    @phase_ts.setter
    def phase_ts(self, ts):
        """Phase stamps on (an int64 [65*64*16] device tensor: the launches then run
        the instrumented build) or off (None)."""
        self._plan.set_phase_ts(ts)
        self._phase_ts = ts

    def error(self) -> int:
        return int(self.err.item())

    def run(self, steps: int, events: Optional[list] = None, lookahead: Optional[int] = None):
        """The next `steps` steps (`StagePlanner.run`); `events` receives one
        (timing event, steps) pair per compute launch."""
        record = None
        if events is not None:
            main = torch.cuda.current_stream()

            def record(n):
                ev = torch.cuda.Event(enable_timing=True)
                ev.record(main)
                events.append((ev, n))
        self._stage.run(steps, lookahead, record)
        self.t.shadows_stale = True

    def step_times_ms(self, first: int, last: int) -> np.ndarray:
        """Per-step durations (ms) of global steps [first, last) from the device stamps."""
        if last - first >= self.TS_RING:
            first = last - self.TS_RING + 1
        ts = self.step_ts.cpu().numpy()
        idx = np.arange(first, last + 1) % self.TS_RING
        return np.diff(ts[idx]).astype(np.float64) * 1e-5     # 100 MHz ticks -> ms
