"""ono_push_settle_f32: the compressor's size rule (compressor.rs:79-89) and the
push's bookkeeping (server_cluster.rs:88-96) applied on the device from the
threshold and the stream length another launch left there.  Bit-exact against
the oracle's f16 codec and grad_drop; neighbours of both operands untouched."""
import numpy as np
import pytest
import torch

from ono_amd import kernels
from conftest import SEED, assert_bitexact
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GUARD = 8
SENTINEL = 0xABCD


def threshold(g, r):
    """calculate_threshold of a SparseCapable{r} push of g (sampled above 16384 values)."""
    t = O.sparse_push(g, r, 0)[1]
    assert t == t and t > 0
    return t


def settle(x, t, nbytes, off_out=0, off_res=0):
    """Run the kernel on copies placed off_* elements into guarded buffers; returns (out16, residual)."""
    n = x.size
    res = torch.full((n + 2 * GUARD,), 7.0, dtype=torch.float32, device="cuda")
    out = torch.full((n + 2 * GUARD,), SENTINEL - 65536, dtype=torch.int16, device="cuda")
    a, b = GUARD + off_res, GUARD + off_out
    res[a:a + n] = torch.from_numpy(x).cuda()
    t_dev = torch.tensor([t], dtype=torch.float32, device="cuda")
    nb_dev = torch.tensor([nbytes], dtype=torch.int64, device="cuda")
    kernels.push_settle(out[b:b + n], res[a:a + n], t_dev, nb_dev)
    torch.cuda.synchronize()
    res_h = res.cpu().numpy()
    out_h = out.cpu().numpy().view(np.uint16)
    assert np.all(res_h[:a] == 7.0) and np.all(res_h[a + n:] == 7.0), "residual neighbours written"
    assert np.all(out_h[:b] == SENTINEL) and np.all(out_h[b + n:] == SENTINEL), "out16 neighbours written"
    return out_h[b:b + n], res_h[a:a + n]


def expect(x, t, nbytes):
    n = x.size
    if nbytes <= 2 * n:
        res = x.copy()
        res[np.abs(x) >= np.float32(t)] = 0.0  # NaN never compares: it stays
        return np.full(n, SENTINEL, np.uint16), res
    return O.f16_encode(x), np.zeros(n, np.float32)


def check(x, t, nbytes, **off):
    out, res = settle(x, t, nbytes, **off)
    e_out, e_res = expect(x, t, nbytes)
    assert np.array_equal(out, e_out), f"out16 differs (nbytes {nbytes}, n {x.size})"
    assert_bitexact(res, e_res, f"residual (nbytes {nbytes}, n {x.size})")


@pytest.mark.parametrize("special", [False, True], ids=["synth", "special"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 2051, 109386])
def test_push_settle_both_branches(n, special):
    x = (O.synth_special if special else O.synth)(n, SEED + 5, 2)
    for r in (0.1, 0.9):
        t = threshold(np.nan_to_num(x, nan=0.0), r)
        drop = len(O.grad_drop(x, t))
        for nbytes in (drop, 2 * n, 2 * n + 2, 8):
            check(x, t, nbytes)


@pytest.mark.parametrize("off_out,off_res", [(1, 1), (1, 0), (0, 1), (2, 3), (3, 3)])
@pytest.mark.parametrize("n", [5, 2051])
def test_push_settle_offset_pointers(n, off_out, off_res):
    """Pointers one element (and more) off a vector boundary: equal phases keep the vector body
    behind a scalar head, different ones take the scalar form."""
    x = O.synth_special(n, SEED + 6, 1)
    t = threshold(O.synth(n, SEED + 6, 1), 0.1)
    for nbytes in (2 * n, 2 * n + 2):
        check(x, t, nbytes, off_out=off_out, off_res=off_res)


@pytest.mark.parametrize("kept,sparse", [(8, True), (9, False)])
def test_push_settle_boundary_is_inclusive(kept, sparse):
    """n = 16: 8 contiguous kept values are a 32-byte stream = 2 n, which still goes sparse;
    9 are 34 bytes and go dense."""
    n, t = 16, 1.0
    x = np.full(n, 0.25, np.float32)
    x[3:3 + kept] = np.arange(2, 2 + kept, dtype=np.float32) * np.where(np.arange(kept) % 2, -1, 1)
    stream = O.grad_drop(x, t)
    assert len(stream) == 8 + 8 + 2 * kept
    assert (len(stream) <= 2 * n) == sparse
    out, res = settle(x, t, len(stream))
    if sparse:
        e = x.copy()
        e[3:3 + kept] = 0.0
        assert np.all(out == SENTINEL)
        assert_bitexact(res, e, "sent values leave the residual")
    else:
        assert np.array_equal(out, O.f16_encode(x))
        assert_bitexact(res, np.zeros(n, np.float32), "dense: the whole residual")


def test_push_settle_behind_the_stream_ordered_drop():
    """The words as the push leaves them: the threshold in a device float, the length written by
    ono_sparse_drop_async — no host wait between the drop and the settle."""
    import ono_amd
    n = 20000
    lib = ono_amd.lib()
    cap = lib.ono_sparse_max_bytes(n)
    for r in (0.1, 0.9):
        x = O.synth(n, SEED + 8, 4)
        t = threshold(x, r)
        res = torch.from_numpy(x).cuda()
        out = torch.full((n,), SENTINEL - 65536, dtype=torch.int16, device="cuda")
        buf = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        t_dev = torch.tensor([t], dtype=torch.float32, device="cuda")
        nb = torch.zeros(1, dtype=torch.int64, device="cuda")
        s = kernels.stream_handle()
        ono_amd._lib.call("ono_sparse_drop_async", buf.data_ptr(), cap, nb.data_ptr(), res.data_ptr(), n, t, s)
        kernels.push_settle(out, res, t_dev, nb)
        ono_amd._lib.call("ono_sparse_drop_check", s)
        stream = O.grad_drop(x, t)
        assert int(nb.item()) == len(stream)
        assert bytes(buf[:len(stream)].cpu().numpy()) == stream
        e_out, e_res = expect(x, t, len(stream))
        assert np.array_equal(out.cpu().numpy().view(np.uint16), e_out)
        assert_bitexact(res.cpu().numpy(), e_res, f"r {r}")
        assert (len(stream) <= 2 * n) == (r == 0.1)
