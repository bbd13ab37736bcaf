#!/usr/bin/env python3
"""A/B of the parameter-server push: ono_cluster_push_grads (threshold, stream-ordered drop and the
settle kernel enqueued back to back for every server, one host wait) against the same frames made by
the blocking public calls per server in sequence (ono_sparse_threshold, ono_sparse_drop, then
ono_sparse_mask or ono_f16_encode_zero, a D2H of the payload, the send).

Both sides run in this process in alternating passes, each push into sockets drained by threads, from
the same residuals (restored before every push, outside the timed window); the first push of each side
is captured and the frames compared.  Workloads: S = 4 x 27,346 values (the config-1 model split) and
S = 2 x 8 Mi values, SparseCapable{0.1}.  Side B pays its ctypes calls (a few per server).

Also, informational: Synchronizer::step on a 16 Mi store from the f16 payload and from the SparseGrad
stream of the same gradient (host-fed, NoBlockingSync, GD).

    python tools/ps_push_ab.py --out profiles/ps_push_ab.txt
"""
import argparse
import ctypes as C
import json
import os
import socket
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oxidized-neural-orchestra_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ono_amd  # noqa: E402
from ono_amd import kernels  # noqa: E402
from ono_amd._lib import call  # noqa: E402
from oracle import oracle as O  # noqa: E402

SEED = 0x0402026
SAMPLE = 16384


class Drain(threading.Thread):
    """Reads and drops everything the socket gets; keeps the bytes while .keep is set."""

    def __init__(self, sock):
        super().__init__(daemon=True)
        self.sock, self.keep, self.kept = sock, False, bytearray()
        self.buf = bytearray(1 << 20)

    def run(self):
        view = memoryview(self.buf)
        while True:
            try:
                k = self.sock.recv_into(view)
            except OSError:
                return
            if k == 0:
                return
            if self.keep:
                self.kept += view[:k]


def frames_of(blob: bytes):
    out, i = [], 0
    while i < len(blob):
        ln = int.from_bytes(blob[i:i + 8], "big")
        out.append(bytes(blob[i:i + 8 + ln]))
        i += 8 + ln
    return out


class BlockingChain:
    """Side B: the public blocking calls per server, in sequence."""

    def __init__(self, sizes, socks, ratio, seed):
        self.sizes, self.socks, self.ratio = sizes, socks, ratio
        self.lib = ono_amd.lib()
        self.state = [C.c_uint64(seed) for _ in sizes]
        self.idx = np.empty(SAMPLE, np.uint32)
        self.res = [torch.empty(n, dtype=torch.float32, device="cuda") for n in sizes]
        self.cap = [self.lib.ono_sparse_max_bytes(n) for n in sizes]
        self.buf = [torch.empty(c, dtype=torch.uint8, device="cuda") for c in self.cap]
        self.out16 = [torch.empty(n, dtype=torch.int16, device="cuda") for n in sizes]
        self.tx = [torch.empty(12 + 2 * n, dtype=torch.uint8).pin_memory() for n in sizes]
        self.tx_np = [t.numpy() for t in self.tx]

    def restore(self, saved):
        for r, s in zip(self.res, saved):
            r.copy_(s)

    def push(self, is_last=False):
        s = kernels.stream_handle()
        for j, n in enumerate(self.sizes):
            res, t, nb = self.res[j], C.c_float(), C.c_size_t()
            if n > SAMPLE:
                call("ono_sparse_sample_default", C.byref(self.state[j]), n, self.idx.ctypes.data, SAMPLE)
                call("ono_sparse_threshold", C.byref(t), res.data_ptr(), n, self.idx.ctypes.data, SAMPLE, self.ratio, s)
            else:
                call("ono_sparse_threshold", C.byref(t), res.data_ptr(), n, None, n, self.ratio, s)
            call("ono_sparse_drop", self.buf[j].data_ptr(), self.cap[j], C.byref(nb), res.data_ptr(), n, t.value, s)
            if nb.value <= 2 * n:
                call("ono_sparse_mask", res.data_ptr(), n, t.value, 1, s)
                pay, kind, src = nb.value, 4 if is_last else 3, self.buf[j][:nb.value]
            else:
                call("ono_f16_encode_zero", self.out16[j].data_ptr(), res.data_ptr(), n, s)
                pay, kind, src = 2 * n, 2 if is_last else 1, self.out16[j].view(torch.uint8)
            self.tx[j][12:12 + pay].copy_(src, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            self.tx_np[j][:8] = np.frombuffer((4 + pay).to_bytes(8, "big"), np.uint8)
            self.tx_np[j][8:12] = np.frombuffer(kind.to_bytes(4, "big"), np.uint8)
            self.socks[j].sendall(memoryview(self.tx_np[j])[:12 + pay])


def spread(xs):
    return {"median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs), "passes": [round(x, 2) for x in xs]}


def workload(name, sizes, ratio, passes, iters, log):
    links = [socket.socketpair() for _ in sizes + sizes]
    a_links, b_links = links[:len(sizes)], links[len(sizes):]
    drains = [Drain(b) for _, b in links]
    for d in drains:
        d.start()
    saved = [torch.from_numpy(O.synth(n, SEED + 7, j)).cuda() for j, n in enumerate(sizes)]
    flat = torch.cat(saved)
    cl = ono_amd.ServerClusterManager(sizes, [a for a, _ in a_links])
    cl.set_sparse(ratio, 0)
    bc = BlockingChain(sizes, [a for a, _ in b_links], ratio, 0)

    def run_a(k):
        tot = 0.0
        for _ in range(k):
            cl.residual_flat.copy_(flat)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cl.push_grads()
            tot += time.perf_counter() - t0
        return tot / k * 1e6

    def run_b(k):
        tot = 0.0
        for _ in range(k):
            bc.restore(saved)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bc.push()
            tot += time.perf_counter() - t0
        return tot / k * 1e6

    # the first push of each side, captured: the same frames, the same residuals
    for d in drains:
        d.keep = True
    run_a(1)
    run_b(1)
    time.sleep(0.2)  # the drains catch up
    for d in drains:
        d.keep = False
    fa = [frames_of(d.kept) for d in drains[:len(sizes)]]
    fb = [frames_of(d.kept) for d in drains[len(sizes):]]
    same = fa == fb and all(len(f) == 1 for f in fa)
    same_res = all(torch.equal(x, y) for x, y in zip(cl.residuals, bc.res))
    kinds = [f[0][11] for f in fa]
    for _ in range(2):  # warm-up of both
        run_a(iters)
        run_b(iters)
    a, b = [], []
    for _ in range(passes):
        a.append(run_a(iters))
        b.append(run_b(iters))
    rec = {"workload": name, "sizes": sizes, "ratio": ratio, "iters_per_pass": iters, "frames_equal": bool(same),
           "residuals_equal": bool(same_res), "frame_kinds": kinds, "frame_bytes": [len(f[0]) for f in fa],
           "single_wait": spread(a), "blocking_chain": spread(b)}
    log(json.dumps(rec))
    cl.close()
    for x, y in links:
        x.close()
        y.close()
    return rec


def step_16mi(log, iters=5):
    n = 16 << 20
    g = O.synth(n, SEED + 9, 1)
    h = O.f16_encode(g)
    stream = np.frombuffer(O.grad_drop(g, O.sparse_push(g, 0.1, 0)[1]), np.uint8).copy()
    store = ono_amd.BlockingStore(ono_amd.shard_size_for(n), 1, np.zeros(n, np.float32), ono_amd.GradientDescent(0.1))
    sync = ono_amd.NoBlockingSync()
    p = np.empty(n, np.float32)
    out = {}
    for name, fn in (("step_f16", lambda: sync.step_f16(store, h, p)), ("step_sparse", lambda: sync.step_sparse(store, stream, p)),
                     ("accumulate_f16", lambda: store.accumulate_f16(h)), ("accumulate_sparse", lambda: store.accumulate_sparse(stream))):
        fn()
        ts = []
        for _ in range(iters):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}
    out.update({"nparams": n, "f16_bytes": int(h.nbytes), "sparse_bytes": int(stream.size)})
    log(json.dumps({"step_16mi": out}))
    sync.drop()
    store.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--passes", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"# ps_push_ab: {torch.cuda.get_device_name(0)}, passes {args.passes}, alternating single_wait / blocking_chain")
    workload("config1_split_4x27346", [27346] * 4, 0.1, args.passes, 200, log)
    workload("2x8Mi", [8 << 20] * 2, 0.1, args.passes, 8, log)
    step_16mi(log)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
