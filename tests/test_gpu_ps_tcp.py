"""Parameter-server mode on the TCP edge: ono_server_task_* (pserver.rs:105-163) and
ono_cluster_* (server_cluster.rs:7-105) over socket pairs, in one process.

End to end the parameters and every worker's residuals follow the oracle composition
(sparse_push / grad_drop / grad_lift / f16 codec / Store) bit for bit; against a peer
written here the frames are the reference's byte for byte."""
import socket
import threading

import numpy as np
import pytest
import torch

import ono_amd
from ono_amd import GradientDescentWithMomentum
from conftest import SEED, assert_bitexact
from oracle import oracle as O

pytestmark = pytest.mark.gpu

JOIN_S = 60
SIZES = [20000, 1031]  # one bucket above 16384 values: its threshold is sampled


class Runner(threading.Thread):
    """fn() on a thread; the exception it raised, if any, in .err."""

    def __init__(self, fn):
        super().__init__(daemon=True)
        self.fn, self.err = fn, None

    def run(self):
        try:
            self.fn()
        except BaseException as e:  # noqa: BLE001 (reported by the test)
            self.err = e


def join_all(threads, aborters):
    """Join with a timeout; abort everything when one fails or hangs, then report."""
    for t in threads:
        t.join(JOIN_S)
        if t.is_alive() or t.err is not None:
            break
    bad = [t for t in threads if t.is_alive() or t.err is not None]
    if bad:
        for a in aborters:
            a.abort()
        for t in threads:
            t.join(10)
    return bad


def frame(kind: int, payload: bytes) -> bytes:
    return (4 + len(payload)).to_bytes(8, "big") + kind.to_bytes(4, "big") + payload


def params_frame(p) -> bytes:
    return frame(5, np.ascontiguousarray(p, dtype="<f4").tobytes())


def recv_exact(sock, n):
    out = b""
    while len(out) < n:
        got = sock.recv(n - len(out))
        assert got, "peer closed"
        out += got
    return out


def recv_frame(sock):
    head = recv_exact(sock, 8)
    return head + recv_exact(sock, int.from_bytes(head, "big"))


def expect_push(chunk, r, state=0, is_last=False):
    """The frame a SparseCapable{r} handle pushes for `chunk` (compressor.rs:71-98), the threshold
    when it went sparse, and the sampler's next state."""
    sparse, t, state = O.sparse_push(chunk, r, state)
    if sparse:
        return frame(4 if is_last else 3, O.grad_drop(chunk, t)), t, state
    return O.frame_dense(O.f16_encode(chunk), is_last), None, state


def pair():
    a, b = socket.socketpair()
    for s in (a, b):
        s.settimeout(JOIN_S)  # the test's own reads fail instead of hanging
    return a, b


def make_store(init, nworkers):
    return ono_amd.BlockingStore(ono_amd.shard_size_for(init.size), nworkers, init, GradientDescentWithMomentum(0.1, 0.9))


def make_ref(init, nworkers):
    return O.Store(init, 7, nworkers, "momentum", lr=0.1, momentum=0.9)


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize("ratio", [0.1, 0.9])
def test_two_servers_two_workers_end_to_end(ratio):
    """2 GPU servers (BarrierSync over 2 worker tasks each) and 2 GPU cluster workers — worker 0
    SparseCapable{ratio} seed 0, worker 1 Base — for 4 rounds, the last is_last.  ratio 0.9 takes the
    compressor's dense fallback on this distribution."""
    nservers, nworkers, rounds = len(SIZES), 2, 4
    inits = [O.synth(n, SEED + 60 + j, 9) for j, n in enumerate(SIZES)]
    stores = [make_store(inits[j], nworkers) for j in range(nservers)]
    syncs = [ono_amd.BarrierSync(nworkers) for _ in range(nservers)]
    links = [[pair() for _ in range(nservers)] for _ in range(nworkers)]  # [w][j] = (worker end, server end)
    tasks = [ono_amd.ServerTask(syncs[j], stores[j], links[w][j][1], timeout_s=JOIN_S)
             for j in range(nservers) for w in range(nworkers)]
    mgrs = [ono_amd.ServerClusterManager(SIZES, [links[w][j][0] for j in range(nservers)], timeout_s=JOIN_S)
            for w in range(nworkers)]
    mgrs[0].set_sparse(ratio, 0)
    grads = [[[O.synth(SIZES[j], SEED + 100 * r + 10 * w + j, w) for j in range(nservers)] for r in range(rounds)]
             for w in range(nworkers)]
    seen_params = [[None] * rounds for _ in range(nworkers)]
    seen_res = [[None] * rounds for _ in range(nworkers)]

    def worker(w):
        m = mgrs[w]
        for r in range(rounds):
            m.pull_params()
            torch.cuda.synchronize()
            seen_params[w][r] = [p.cpu().numpy().copy() for p in m.params]
            for j in range(nservers):
                m.grads[j].copy_(torch.from_numpy(grads[w][r][j]))
            m.acc_residual()
            m.push_grads(is_last=r == rounds - 1)
            seen_res[w][r] = [x.cpu().numpy().copy() for x in m.residuals]

    threads = [Runner(t.run) for t in tasks] + [Runner(lambda w=w: worker(w)) for w in range(nworkers)]
    try:
        for t in threads:
            t.start()
        bad = join_all(threads, tasks + mgrs)
        assert not bad, [(t.err, t.is_alive()) for t in bad]
    finally:
        for m in mgrs:
            m.close()
        for t in tasks:
            t.close()
        for s in syncs:
            s.drop()
        for row in links:
            for a, b in row:
                a.close()
                b.close()

    refs = [make_ref(inits[j], nworkers) for j in range(nservers)]
    res = [[np.zeros(n, np.float32) for n in SIZES] for _ in range(nworkers)]
    states = [0] * nservers  # every handle of worker 0 starts its own sampler stream at the seed
    went_sparse = 0
    for r in range(rounds):
        for w in range(nworkers):
            for j in range(nservers):
                assert_bitexact(seen_params[w][r][j], refs[j].pull_params(), f"params round {r} worker {w} server {j}")
        for j in range(nservers):
            for w in range(nworkers):
                res[w][j] = res[w][j] + grads[w][r][j]
                x = res[w][j]
                sparse, t = False, None
                if w == 0:
                    sparse, t, states[j] = O.sparse_push(x, ratio, states[j])
                if sparse:
                    went_sparse += 1
                    refs[j].accumulate(O.grad_lift(O.grad_drop(x, t), cap=x.size))
                    x[np.abs(x) >= np.float32(t)] = 0.0
                else:
                    refs[j].accumulate(O.f16_decode(O.f16_encode(x)))
                    x[:] = 0.0
                assert_bitexact(seen_res[w][r][j], x, f"residual round {r} worker {w} server {j}")
            refs[j].update_params()
    assert went_sparse == (rounds * nservers if ratio == 0.1 else 0)
    for j in range(nservers):  # the is_last gradients were stepped too
        assert_bitexact(stores[j].pull_params(), refs[j].pull_params(), f"final params server {j}")


# ---------------------------------------------------------------- byte-exact frames
def test_server_frames_under_a_reference_style_worker():
    """A GPU server task under a worker written here: the Params frames are the expected bytes after a
    DenseGrad, a SparseGrad, and a correct gradient behind two of the wrong length (which get no
    answer); the is_last gradient is stepped and answered by nothing."""
    n = 4099
    init = O.synth(n, SEED + 70, 9)
    store, ref = make_store(init, 1), make_ref(init, 1)
    sync = ono_amd.BarrierSync(1)
    mine, theirs = pair()
    task = ono_amd.ServerTask(sync, store, theirs, timeout_s=JOIN_S)
    run = Runner(task.run)
    run.start()
    try:
        assert recv_frame(mine) == params_frame(init)

        g = O.synth(n, SEED + 71, 1)
        mine.sendall(O.frame_dense(O.f16_encode(g)))
        ref.accumulate(O.f16_decode(O.f16_encode(g)))
        ref.update_params()
        assert recv_frame(mine) == params_frame(ref.pull_params())

        g = O.synth(n, SEED + 72, 1)
        f, t, _ = expect_push(g, 0.1)
        assert t is not None
        mine.sendall(f)
        ref.accumulate(O.grad_lift(O.grad_drop(g, t), cap=n))
        ref.update_params()
        assert recv_frame(mine) == params_frame(ref.pull_params())

        # wrong lengths: a DenseGrad of n - 1 values, a SparseGrad whose total is n + 1; then a correct one
        mine.sendall(O.frame_dense(O.f16_encode(g[:-1])))
        mine.sendall(frame(3, O.grad_drop(np.append(g, np.float32(1.0)), t)))
        g = O.synth(n, SEED + 73, 1)
        mine.sendall(O.frame_dense(O.f16_encode(g)))
        ref.accumulate(O.f16_decode(O.f16_encode(g)))
        ref.update_params()
        assert recv_frame(mine) == params_frame(ref.pull_params())  # the one answer

        g = O.synth(n, SEED + 74, 1)
        f, t, _ = expect_push(g, 0.1, is_last=True)
        mine.sendall(f)
        ref.accumulate(O.grad_lift(O.grad_drop(g, t), cap=n))
        ref.update_params()
        run.join(JOIN_S)
        assert not run.is_alive() and run.err is None, run.err
        mine.setblocking(False)
        with pytest.raises(BlockingIOError):  # no parameters after an is_last gradient
            mine.recv(1)
        assert_bitexact(store.pull_params(), ref.pull_params(), "the is_last gradient was stepped")
    finally:
        task.abort()
        run.join(10)
        task.close()
        sync.drop()
        mine.close()
        theirs.close()


@pytest.mark.parametrize("ratio", [0.0, 0.1, 0.9])
def test_cluster_frames_under_reference_style_servers(ratio):
    """A GPU cluster worker against servers written here: it takes their Params frames into its
    buckets and pushes exactly the frames of the reference's serializer, two rounds (the second
    is_last), the samplers' streams and the residuals carried."""
    links = [pair() for _ in SIZES]
    m = ono_amd.ServerClusterManager(SIZES, [a for a, _ in links], timeout_s=JOIN_S)
    m.set_sparse(ratio, 5)
    states = [5] * len(SIZES)
    res = [np.zeros(n, np.float32) for n in SIZES]
    try:
        for rnd in range(2):
            sent = [O.synth(n, SEED + 80 + rnd, j) for j, n in enumerate(SIZES)]
            for (_, b), p in zip(links, sent):
                b.sendall(params_frame(p))
            m.pull_params()
            for j, p in enumerate(sent):
                assert_bitexact(m.params[j].cpu().numpy(), p, f"params server {j}")
            for j, n in enumerate(SIZES):
                m.grads[j].copy_(torch.from_numpy(O.synth(n, SEED + 90 + rnd, j)))
                res[j] = res[j] + O.synth(n, SEED + 90 + rnd, j)
            m.acc_residual()
            push = Runner(lambda: m.push_grads(is_last=rnd == 1))
            push.start()
            frames = [recv_frame(b) for _, b in links]
            push.join(JOIN_S)
            assert not push.is_alive() and push.err is None, push.err
            for j in range(len(SIZES)):
                if ratio:
                    f, t, states[j] = expect_push(res[j], ratio, states[j], is_last=rnd == 1)
                else:
                    f, t = O.frame_dense(O.f16_encode(res[j]), rnd == 1), None
                assert frames[j] == f, f"round {rnd} server {j}: frame of kind {frames[j][11]}, {len(frames[j])} bytes"
                if t is None:
                    res[j][:] = 0.0
                else:
                    res[j][np.abs(res[j]) >= np.float32(t)] = 0.0
                assert_bitexact(m.residuals[j].cpu().numpy(), res[j], f"round {rnd} residual server {j}")
    finally:
        m.abort()
        m.close()
        for a, b in links:
            a.close()
            b.close()


def test_cluster_caller_sampler_is_used_above_the_sample_size():
    """An installed sampler draws the threshold sample of a bucket above 16384 values (and is called,
    its indices unused, for a smaller one)."""
    links = [pair() for _ in SIZES]
    m = ono_amd.ServerClusterManager(SIZES, [a for a, _ in links], timeout_s=JOIN_S)
    m.set_sparse(0.1, 0)
    calls = []

    def sampler(length, amount):
        calls.append((length, amount))
        return np.arange(amount, dtype=np.uint32) * (length // amount)

    for j in range(len(SIZES)):
        m.set_sampler(j, sampler)
    try:
        xs = [O.synth(n, SEED + 95, j) for j, n in enumerate(SIZES)]
        for j, x in enumerate(xs):
            m.residuals[j].copy_(torch.from_numpy(x))
        push = Runner(lambda: m.push_grads())
        push.start()
        frames = [recv_frame(b) for _, b in links]
        push.join(JOIN_S)
        assert push.err is None and not push.is_alive(), push.err
        assert calls == [(SIZES[0], 16384), (SIZES[1], SIZES[1])]
        t0 = O.sparse_threshold_sample(xs[0], 0.1, np.arange(16384, dtype=np.uint32) * (SIZES[0] // 16384))
        assert frames[0] == frame(3, O.grad_drop(xs[0], t0))
        assert frames[1] == frame(3, O.grad_drop(xs[1], O.sparse_threshold(xs[1], 0.1)))
    finally:
        m.abort()
        m.close()
        for a, b in links:
            a.close()
            b.close()


# ------------------------------------------------------------------------- errors
def server_under_test(n=1031):
    init = O.synth(n, SEED + 75, 9)
    store = make_store(init, 1)
    sync = ono_amd.BarrierSync(1)
    mine, theirs = pair()
    task = ono_amd.ServerTask(sync, store, theirs, timeout_s=JOIN_S)
    run = Runner(task.run)
    run.start()
    assert recv_frame(mine) == params_frame(init)

    def cleanup():
        task.abort()
        run.join(10)
        task.close()
        sync.drop()
        mine.close()
        theirs.close()
    return init, store, task, run, mine, cleanup


@pytest.mark.parametrize("what", ["params", "data chunk", "done", "upgraded"])
def test_server_refuses_other_messages(what):
    init, store, task, run, mine, cleanup = server_under_test()
    try:
        mine.sendall({"params": params_frame(init), "data chunk": frame(6, b"\x00" * 16),
                      "done": frame(0, b'"done"'), "upgraded": frame(0, b'"upgraded"')}[what])
        run.join(JOIN_S)
        assert not run.is_alive()
        assert isinstance(run.err, ono_amd.InvalidWorkerEvent) and "invalid message" in str(run.err), run.err
        assert_bitexact(store.pull_params(), init, "store untouched")
    finally:
        cleanup()


def test_server_keeps_the_loss_diverged_error():
    init, store, task, run, mine, cleanup = server_under_test()
    try:
        mine.sendall(frame(0, b'{"report_loss":{"losses":[0.5,null]}}'))
        run.join(JOIN_S)
        assert not run.is_alive()
        assert isinstance(run.err, ono_amd.IoError) and "loss diverged" in str(run.err), run.err
    finally:
        cleanup()


def test_server_reports_a_malformed_sparse_stream_of_the_right_total():
    n = 1031
    init, store, task, run, mine, cleanup = server_under_test(n)
    try:
        g = O.synth(n, SEED + 76, 1)
        mine.sendall(frame(3, O.grad_drop(g, O.sparse_threshold(g, 0.1))[:-1]))
        run.join(JOIN_S)
        assert not run.is_alive()
        assert isinstance(run.err, ono_amd.InvalidWorkerEvent) and "Truncated float data" in str(run.err), run.err
        assert_bitexact(store.pull_params(), init, "store untouched")
    finally:
        cleanup()


def test_server_peer_closed_mid_frame():
    init, store, task, run, mine, cleanup = server_under_test()
    try:
        f = O.frame_dense(O.f16_encode(O.synth(init.size, SEED + 77, 1)))
        mine.sendall(f[:len(f) // 2])
        mine.close()
        run.join(JOIN_S)
        assert not run.is_alive()
        assert isinstance(run.err, ono_amd.IoError) and "closed the connection" in str(run.err), run.err
    finally:
        cleanup()


def test_abort_unblocks_a_waiting_server_task():
    init, store, task, run, mine, cleanup = server_under_test()
    try:
        assert run.is_alive()  # waiting for a gradient that never comes
        task.abort()
        run.join(JOIN_S)
        assert not run.is_alive()
        assert isinstance(run.err, ono_amd.Aborted), run.err
    finally:
        cleanup()


def test_cluster_pull_params_errors_and_abort():
    links = [pair() for _ in SIZES]
    m = ono_amd.ServerClusterManager(SIZES, [a for a, _ in links], timeout_s=JOIN_S)
    try:
        # a DenseGrad where the Params of server 1 are expected
        links[0][1].sendall(params_frame(np.zeros(SIZES[0], np.float32)))
        links[1][1].sendall(O.frame_dense(np.zeros(SIZES[1], np.uint16)))
        with pytest.raises(ono_amd.IoError, match="Expected params from server 1"):
            m.pull_params()
        # Params of another length
        links[0][1].sendall(params_frame(np.zeros(SIZES[0] + 1, np.float32)))
        with pytest.raises(ono_amd.SizeMismatch):
            m.pull_params()
        # the connection is still framed: a good pull after both
        ps = [O.synth(n, SEED + 85, j) for j, n in enumerate(SIZES)]
        for (_, b), p in zip(links, ps):
            b.sendall(params_frame(p))
        m.pull_params()
        for j, p in enumerate(ps):
            assert_bitexact(m.params[j].cpu().numpy(), p, f"params server {j}")
        # a peer that closes mid-frame
        f = params_frame(ps[0])
        links[0][1].sendall(f[:100])
        links[0][1].close()
        with pytest.raises(ono_amd.IoError, match="closed the connection"):
            m.pull_params()
    finally:
        m.abort()
        m.close()
        for a, b in links:
            a.close()
            b.close()
    # abort unblocks a pull that waits for parameters nobody sends
    links = [pair() for _ in SIZES]
    m = ono_amd.ServerClusterManager(SIZES, [a for a, _ in links], timeout_s=JOIN_S)
    pull = Runner(m.pull_params)
    try:
        pull.start()
        m.abort()
        pull.join(JOIN_S)
        assert not pull.is_alive()
        assert isinstance(pull.err, ono_amd.Aborted), pull.err
    finally:
        m.abort()
        pull.join(10)
        m.close()
        for a, b in links:
            a.close()
            b.close()
