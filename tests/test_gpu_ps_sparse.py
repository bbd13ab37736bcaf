"""The SparseGrad arm of the parameter-server receive on the device:
ono_store_accumulate_sparse{,_dev} and ono_sync_step_sparse against the oracle
composition grad_lift (sparse/protocol.rs:96-144) -> Store::accumulate
(handles/worker.rs:102-108 feeding Synchronizer::step).  Bit-exact."""
import threading

import numpy as np
import pytest
import torch

import ono_amd
from ono_amd import Adam, GradientDescent, GradientDescentWithMomentum
from conftest import SEED, assert_bitexact
from oracle import oracle as O

pytestmark = pytest.mark.gpu

OPTS = {
    "gd": GradientDescent(0.1),
    "momentum": GradientDescentWithMomentum(0.1, 0.9),
    "adam": Adam(0.1, 0.9, 0.999, 1e-8),
}
SIZES = [1, 5, 4099, 109386]


def oracle_stream(g, which):
    """A grad_drop stream of g: the SparseCapable{0.1} push, every value (one run), or none (8 bytes)."""
    if which == "r0.1":
        s = O.grad_drop(g, O.sparse_push(g, 0.1, 0)[1])  # (the threshold of the push, sampled above 16384 values)
        assert len(s) > 8 or g.size < 16
        return s
    if which == "all":
        s = O.grad_drop(g, 0.0)
        assert len(s) == 8 + 8 + 2 * g.size  # one run
        return s
    s = O.grad_drop(g, float("inf"))
    assert len(s) == 8
    return s


def hand_stream(total, runs):
    """[u64 LE total] { [u32 LE gap][u32 LE len][u16 LE x len] }* from (gap, [f16 bits]) pairs."""
    out = int(total).to_bytes(8, "little")
    for gap, vals in runs:
        out += int(gap).to_bytes(4, "little") + len(vals).to_bytes(4, "little")
        out += np.asarray(vals, dtype="<u2").tobytes()
    return out


def feed(store, stream, dev):
    if dev:
        store.accumulate_sparse(torch.frombuffer(bytearray(stream), dtype=torch.uint8).cuda())
    else:
        store.accumulate_sparse(stream)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("which", ["r0.1", "all", "none"])
@pytest.mark.parametrize("nparams", SIZES)
def test_store_accumulate_sparse_vs_oracle(nparams, which, dev):
    init = O.synth(nparams, SEED + 1, 9)
    s = ono_amd.BlockingStore(ono_amd.shard_size_for(nparams), 1, init, OPTS["momentum"])
    ref = O.Store(init, 7, 1, "momentum", lr=0.1, momentum=0.9)
    for rnd in range(2):
        stream = oracle_stream(O.synth(nparams, SEED + rnd, 1), which)
        feed(s, stream, dev)
        ref.accumulate(O.grad_lift(stream, cap=nparams))
        s.update_params()
        ref.update_params()
        assert_bitexact(s.pull_params(), ref.pull_params(), f"{which} round {rnd}")


@pytest.mark.parametrize("kind", ["gd", "momentum", "adam"])
@pytest.mark.parametrize("nparams", [5, 4099])
def test_blocking_store_mixed_pushes_in_one_round(kind, nparams):
    """Two workers whose pushes arrive as f32, f16 and sparse, mixed within a round."""
    init = O.synth(nparams, SEED + 1, 9)
    s = ono_amd.BlockingStore(ono_amd.shard_size_for(nparams), 2, init, OPTS[kind])
    ref = O.Store(init, 7, 2, kind, lr=0.1, momentum=0.9, beta1=0.9, beta2=0.999, eps=1e-8)
    forms = [("f32", "sparse"), ("sparse", "f16"), ("sparse", "sparse"), ("f16", "f32")]
    for rnd, pair in enumerate(forms):
        for w, form in enumerate(pair):
            g = O.synth(nparams, SEED + rnd, w)
            if form == "f32":
                s.accumulate(g)
                ref.accumulate(g)
            elif form == "f16":
                h = O.f16_encode(g)
                s.accumulate_f16(h)
                ref.accumulate(O.f16_decode(h))
            else:
                stream = oracle_stream(g, "r0.1")
                feed(s, stream, dev=bool(w))
                ref.accumulate(O.grad_lift(stream, cap=nparams))
        s.update_params()
        ref.update_params()
        assert_bitexact(s.pull_params(), ref.pull_params(), f"{kind} round {rnd}")


@pytest.mark.parametrize("nparams", [5, 4099])
def test_wild_store_momentum_decays_on_unsent_positions(nparams):
    """The lifted zeros pass through the optimizer (wild/shard.rs:43-58): the velocity of a
    position that was not sent keeps decaying and moving its parameter."""
    init = O.synth(nparams, SEED + 1, 9)
    s = ono_amd.WildStore(ono_amd.shard_size_for(nparams), init, OPTS["momentum"])
    ref = O.WildStore(init, 7, "momentum", lr=0.1, momentum=0.9)
    for rnd in range(4):
        stream = oracle_stream(O.synth(nparams, SEED + rnd, 2), "r0.1")
        feed(s, stream, dev=bool(rnd % 2))
        ref.accumulate(O.grad_lift(stream, cap=nparams))
        assert_bitexact(s.pull_params(), ref.pull_params(), f"round {rnd}")


def _one_round(s, ref, nparams, seed):
    g = O.synth(nparams, seed, 3)
    stream = oracle_stream(g, "r0.1")
    s.accumulate_sparse(stream)
    ref.accumulate(O.grad_lift(stream, cap=nparams))
    s.update_params()
    ref.update_params()
    assert_bitexact(s.pull_params(), ref.pull_params(), "the round after")


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_hand_built_streams(dev):
    nparams = 4099
    init = O.synth(nparams, SEED + 1, 9)
    s = ono_amd.BlockingStore(ono_amd.shard_size_for(nparams), 1, init, OPTS["gd"])
    ref = O.Store(init, 7, 1, "gd", lr=0.1)
    one, two = 0x3C00, 0x4000
    streams = {
        "zero-length run": hand_stream(nparams, [(3, [one, two]), (5, []), (0, [two]), (100, [])]),
        "explicit zeros in a run": hand_stream(nparams, [(7, [one, 0x0000, 0x8000, two, 0x8000]), (4000, [0x0000])]),
        # every other position its own run: 8 + 10 ceil(n / 2) bytes, above 2 bytes per value
        "longer than the f16 payload": hand_stream(nparams, [(0, [one])] + [(1, [0x3800 + (i % 512)])
                                                             for i in range(1, (nparams + 1) // 2)]),
    }
    assert len(streams["longer than the f16 payload"]) > 2 * nparams
    assert len(streams["longer than the f16 payload"]) <= ono_amd.lib().ono_sparse_max_bytes(nparams)
    for what, stream in streams.items():
        feed(s, stream, dev)
        ref.accumulate(O.grad_lift(stream, cap=nparams))
        s.update_params()
        ref.update_params()
        assert_bitexact(s.pull_params(), ref.pull_params(), what)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("kind", ["blocking", "wild"])
def test_refused_streams_leave_the_store_untouched(kind, dev):
    nparams = 4099
    init = O.synth(nparams, SEED + 1, 9)
    if kind == "blocking":
        s = ono_amd.BlockingStore(ono_amd.shard_size_for(nparams), 1, init, OPTS["momentum"])
        ref = O.Store(init, 7, 1, "momentum", lr=0.1, momentum=0.9)
    else:
        s = ono_amd.WildStore(ono_amd.shard_size_for(nparams), init, OPTS["momentum"])
        ref = O.WildStore(init, 7, "momentum", lr=0.1, momentum=0.9)
    _one_round(s, ref, nparams, SEED + 20)
    good = oracle_stream(O.synth(nparams, SEED + 21, 3), "r0.1")
    for total in (nparams - 1, nparams + 1):  # total_len is checked before the lift, well-formed or not
        with pytest.raises(ono_amd.SizeMismatch):
            feed(s, int(total).to_bytes(8, "little") + good[8:], dev)
    with pytest.raises(ono_amd.SizeMismatch):
        feed(s, hand_stream(nparams + 5, []), dev)
    _one_round(s, ref, nparams, SEED + 22)
    with pytest.raises(ono_amd.InvalidWorkerEvent, match="Truncated float data"):
        feed(s, good[:-1], dev)
    with pytest.raises(ono_amd.InvalidWorkerEvent, match="Missing chunk length bytes at grad lift"):
        feed(s, good + b"\x01\x00\x00\x00\x02", dev)
    with pytest.raises(ono_amd.InvalidWorkerEvent, match="Gradient chunk exceeds target vector bounds"):
        feed(s, hand_stream(nparams, [(nparams - 1, [0x3C00, 0x3C00])]), dev)
    with pytest.raises(ono_amd.InvalidWorkerEvent, match="smaller than TOTAL_LEN_SIZE"):
        feed(s, good[:7], dev)
    _one_round(s, ref, nparams, SEED + 23)


def test_barrier_sync_three_workers_f32_f16_sparse():
    """Three worker tasks step through BarrierSync, one per gradient form.  Integer-valued
    gradients (exact in f16), so neither the arrival order nor the wire form changes the sums."""
    nparams, nworkers, rounds = 4099, 3, 4
    init = O.synth(nparams, SEED, 0)
    s = ono_amd.BlockingStore(64, nworkers, init, GradientDescent(0.1))
    sync = ono_amd.BarrierSync(nworkers)
    clones = [sync.clone() for _ in range(nworkers - 1)] + [sync]
    grads = [[np.clip(np.round(O.synth(nparams, SEED + r, w) * 64), -1024, 1024).astype(np.float32)
              for r in range(rounds)] for w in range(nworkers)]
    # worker 2 sends the values at or above its threshold only: what the server adds is the lift of its stream
    streams = [oracle_stream(grads[2][r], "r0.1") for r in range(rounds)]
    outs = [[None] * rounds for _ in range(nworkers)]
    errors = []

    def worker(w):
        try:
            p = np.empty(nparams, np.float32)
            for r in range(rounds):
                if w == 0:
                    clones[w].step(s, grads[w][r], p)
                elif w == 1:
                    clones[w].step_f16(s, O.f16_encode(grads[w][r]), p)
                else:
                    clones[w].step_sparse(s, streams[r], p)
                outs[w][r] = p.copy()
        except Exception as e:  # pragma: no cover
            errors.append(e)

    ts = [threading.Thread(target=worker, args=(w,)) for w in range(nworkers)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(60)
    assert not errors and all(not t.is_alive() for t in ts), errors
    ref = O.Store(init, 64, nworkers, "gd", lr=0.1)
    for r in range(rounds):
        ref.accumulate(grads[0][r])
        ref.accumulate(O.f16_decode(O.f16_encode(grads[1][r])))
        ref.accumulate(O.grad_lift(streams[r], cap=nparams))
        ref.update_params()
        e = ref.pull_params()
        for w in range(nworkers):
            assert_bitexact(outs[w][r], e, f"round {r} worker {w}")
    for c in clones:
        c.drop()


def test_step_sparse_refusals_do_not_enter_the_barrier():
    nparams = 1031
    init = O.synth(nparams, SEED, 0)
    s = ono_amd.BlockingStore(64, 1, init, GradientDescent(0.1))
    sync = ono_amd.NoBlockingSync()
    p = np.empty(nparams, np.float32)
    with pytest.raises(ono_amd.SizeMismatch):
        sync.step_sparse(s, hand_stream(nparams + 1, []), p)
    with pytest.raises(ono_amd.InvalidWorkerEvent, match="Truncated float data"):
        sync.step_sparse(s, hand_stream(nparams, [(0, [1, 2])])[:-1], p)
    assert_bitexact(s.pull_params(), init, "untouched")
    g = O.synth(nparams, SEED + 4, 1)
    stream = oracle_stream(g, "r0.1")
    sync.step_sparse(s, stream, p)
    ref = O.Store(init, 64, 1, "gd", lr=0.1)
    ref.accumulate(O.grad_lift(stream, cap=nparams))
    ref.update_params()
    assert_bitexact(p, ref.pull_params(), "step")
    sync.drop()
