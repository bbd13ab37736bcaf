"""Parameter-server mode on the TCP edge.

ServerTask mirrors the per-worker task of ParameterServer::spawn
(parameter_server/src/service/pserver.rs:105-163): an MI355X store under any
worker that speaks the reference's frames.  ServerClusterManager mirrors
worker/src/middlewares/server_cluster.rs:7-105 with its buckets in HBM: an
MI355X worker under any servers.  Both run on the caller's connected sockets
(which stay the caller's and must outlive the object).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import kernels
from ._lib import SAMPLE_FN, call, lib
from .ring import _DevArray
from .store import _Store, _Sync


class ServerTask:
    """One worker's task on the server.  Takes its own clone of `sync`
    (released by close(), which shrinks a BarrierSync as a dropped clone
    does); `run()` blocks until the worker's is_last gradient."""

    def __init__(self, sync: _Sync, store: _Store, sock, timeout_s: float = 600.0):
        h = C.c_void_p()
        call("ono_server_task_create", C.byref(h), sync._h, store._h, sock.fileno(), float(timeout_s))
        self._h, self._sock, self._store = h, sock, store

    def run(self) -> None:
        """Send the parameters, then per received gradient frame: step and send
        the parameters again; returns after an is_last gradient.  Raises
        InvalidWorkerEvent ("invalid message", a malformed sparse stream),
        IoError (socket failure, timeout, "loss diverged") or Aborted."""
        call("ono_server_task_run", self._h)

    def abort(self) -> None:
        call("ono_server_task_abort", self._h)

    def close(self) -> None:
        if getattr(self, "_h", None):
            call("ono_server_task_destroy", self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ServerClusterManager:
    """`socks[j]` is the connection to server j, which holds `sizes[j]`
    parameters.  params / grads / residuals are lists of torch views of the
    per-server buckets; `*_flat` are the contiguous server-major allocations
    they slice."""

    def __init__(self, sizes, socks, *, device: int | None = None, timeout_s: float = 600.0):
        sizes = [int(s) for s in sizes]
        if len(sizes) != len(socks) or not sizes:
            raise ValueError("one socket per server")
        self.device = torch.cuda.current_device() if device is None else device
        self.sizes, self._socks = sizes, list(socks)
        n = len(sizes)
        h = C.c_void_p()
        call("ono_cluster_create", C.byref(h), n, (C.c_size_t * n)(*sizes), (C.c_int * n)(*[s.fileno() for s in socks]),
             self.device, float(timeout_s))
        self._h = h
        self._samplers = {}
        dev, total, L = f"cuda:{self.device}", sum(sizes), lib()
        self.params_flat = torch.as_tensor(_DevArray(L.ono_cluster_params(h, 0), total), device=dev)
        self.grad_flat = torch.as_tensor(_DevArray(L.ono_cluster_grad(h, 0), total), device=dev)
        self.residual_flat = torch.as_tensor(_DevArray(L.ono_cluster_residual(h, 0), total), device=dev)
        offs = np.concatenate([[0], np.cumsum(sizes)])
        self.params = [self.params_flat[offs[j]:offs[j + 1]] for j in range(n)]
        self.grads = [self.grad_flat[offs[j]:offs[j + 1]] for j in range(n)]
        self.residuals = [self.residual_flat[offs[j]:offs[j + 1]] for j in range(n)]

    def set_sparse(self, r: float, seed: int = 0) -> None:
        """Every handle's serializer: SparseCapable{r} (0 = Base); each handle's
        default threshold sampler starts its own stream at `seed`."""
        call("ono_cluster_set_sparse", self._h, float(r), int(seed) & (2 ** 64 - 1))

    def set_sampler(self, server: int, fn) -> None:
        """fn(length, amount) -> `amount` distinct indices of [0, length) for
        handle `server` (see WorkerRingManager.set_sampler); None = default."""
        if fn is None:
            self._samplers.pop(server, None)
            call("ono_cluster_set_sampler", self._h, server, None, None)
            return

        def tramp(_ctx, length, idx, amount):
            try:
                got = np.asarray(fn(int(length), int(amount)), dtype=np.uint32)
                if got.shape != (amount,):
                    return 1
                C.memmove(idx, got.ctypes.data, 4 * amount)
                return 0
            except Exception:
                return 1

        self._samplers[server] = SAMPLE_FN(tramp)  # kept alive as long as the manager
        call("ono_cluster_set_sampler", self._h, server, C.cast(self._samplers[server], C.c_void_p), None)

    def pull_params(self) -> list[torch.Tensor]:
        """One Params frame per server into the params buckets (blocking)."""
        call("ono_cluster_pull_params", self._h)
        return self.params

    def acc_residual(self, stream=None) -> None:
        """residual += grad over every server, one launch."""
        call("ono_cluster_acc_residual", self._h, kernels.stream_handle(stream))

    def push_grads(self, is_last: bool = False) -> None:
        """Every server's residual through its serializer, then the
        bookkeeping of server_cluster.rs:88-96 (blocking).  Work queued on
        torch's current stream (writes to the residual views) completes first."""
        torch.cuda.current_stream().synchronize()
        call("ono_cluster_push_grads", self._h, int(is_last))

    def abort(self) -> None:
        call("ono_cluster_abort", self._h)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self.params = self.grads = self.residuals = None
            self.params_flat = self.grad_flat = self.residual_flat = None
            call("ono_cluster_destroy", self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
