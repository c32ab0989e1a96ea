"""GPU: the uniform seal's pair loop at the edges of its loop split, every body byte against the oracle.

seal_frame's whole-line path (cz_kernels.hip) seals blocks 2k and 2k+1 from payload line k.  The
loop runs two iterations per trip over two register sets while the whole 128-byte line lies inside
the payload, then at most one more such iteration, then at most one last iteration that loads only
the 96 bytes its blocks read.  Which of the three parts run, and how often, depends on
nfull = (n + 33) / 64 and on where the payload ends in its last line; the block counter each part
hands to Salsa20 must stay wave-uniform in the kernels that rotate on the scalar unit, and those
kernels are chosen per wave by the nonce counter's high word.

Batches go through batch.seal_uniform with 16-byte aligned payload slots and body slots of a
128-byte multiple: whole waves take the line-staged kernel (region-staged below 256 body bytes), a
partial last wave the direct stores beside them."""
import numpy as np
import pytest

from cz_testlib import DESC_DTYPE, load_golden, oracle

pytestmark = pytest.mark.gpu

G = load_golden()
PRECOM = bytes.fromhex(G["keys"]["precom"])
GUARD = 4096
COUNTS = (64, 128, 192 + 64, 200)   # whole waves, and 3 waves + 8 frames stored directly
MAXCOUNT = max(COUNTS)

# nfull = 2 .. 6: no pair iteration (2, 3), one (4, 5), two (6)
SPLIT_EDGES = [95, 159, 223, 287, 351]
# the payload ends inside chunk 5, 6, 7 of its last line, and on the line's end
LINE_ENDS = sorted({128 * ((n + 127) // 128 - 1) + e for n in SPLIT_EDGES for e in (88, 104, 120, 128)})
# (n + 33) % 64 = 0, 1, 16, 17, 33, 63 after 16 and after 17 full blocks: 7 / 8 pair iterations
TAILS = [64 * nf - 33 + t for nf in (16, 17) for t in (0, 1, 16, 17, 33, 63)]
SIZES = SPLIT_EDGES + [n for n in LINE_ENDS if n not in SPLIT_EDGES] + TAILS + [4096]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch, torch.device("cuda:0")


@pytest.fixture(scope="module")
def subkeys(torch_dev):
    torch, dev = torch_dev
    from jeromq_amd import _lib, batch
    k = torch.tensor(list(PRECOM), dtype=torch.uint8, device=dev).view(1, 32)
    return torch.cat([batch.subkeys(k, _lib.CZ_DIR_C2S), batch.subkeys(k, _lib.CZ_DIR_S2C)])


def _oracle_bodies(hin, in_stride, count, n, flags, counter0):
    desc = np.zeros(count, dtype=DESC_DTYPE)
    desc["in_off"] = np.arange(count, dtype=np.uint64) * in_stride
    desc["out_off"] = np.arange(count, dtype=np.uint64) * (n + 33)
    desc["len"] = n
    desc["counter"] = np.uint64(counter0) + np.arange(count, dtype=np.uint64)
    desc["flags"] = flags
    out = np.zeros(count * (n + 33), dtype=np.uint8)
    precom = np.frombuffer(PRECOM * 2, dtype=np.uint8)
    oracle().or_seal_batch(desc.ctypes.data, count, hin.ctypes.data, out.ctypes.data, precom.ctypes.data, 0, 8)
    return out.reshape(count, n + 33)


def _check(torch_dev, subkeys, n, counter0, counts=COUNTS):
    """seal `counts` frames of n bytes from one input; the oracle runs once, over the longest batch"""
    torch, dev = torch_dev
    from jeromq_amd import batch
    in_stride = max(16, (n + 15) // 16 * 16)
    out_stride = (n + 33 + 127) // 128 * 128
    d_in = torch.empty(MAXCOUNT * in_stride, dtype=torch.uint8, device=dev)
    batch.fill(d_in, 0x5EA1 + n)
    flags = torch.zeros(MAXCOUNT, dtype=torch.uint8, device=dev)
    flags[::8] = 1                                   # MORE on every 8th frame
    hin, fl = d_in.cpu().numpy(), flags.cpu().numpy()
    want = _oracle_bodies(hin, in_stride, MAXCOUNT, n, fl, counter0)
    for count in counts:
        d_out = torch.full((count * out_stride + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
        batch.seal_uniform(d_in, in_stride, d_out, out_stride, count, n, subkeys[0], counter0, flags8=flags)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert np.all(got[count * out_stride:] == 0xAB), f"n={n} count={count}: bytes after the last slot written"
        bodies = got[:count * out_stride].reshape(count, out_stride)[:, :n + 33]
        bad = np.nonzero(np.any(bodies != want[:count], axis=1))[0]
        assert len(bad) == 0, (f"n={n} count={count} counter0={counter0:#x}: {len(bad)} frames differ, first {bad[:5]}, "
                               f"first byte {np.nonzero(bodies[bad[0]] != want[bad[0]])[0][:4]}")


@pytest.mark.parametrize("n", SIZES)
def test_pair_loop_sizes(torch_dev, subkeys, n):
    _check(torch_dev, subkeys, n, 3)


# 256 - 30: the counter's second-lowest byte changes inside wave 0.  2^32 - 100 and 2^32 - 1: the high
# nonce word changes at frame 100 (wave 1) and at frame 1 (wave 0); those waves hold two values of
# it and take the kernel's per-lane rounds, their neighbours the scalar-unit ones.
@pytest.mark.parametrize("counter0", [256 - 30, 2**32 - 100, 2**32 - 1])
@pytest.mark.parametrize("n", [351, 1024, 4096])
def test_pair_loop_counters(torch_dev, subkeys, n, counter0):
    _check(torch_dev, subkeys, n, counter0, counts=(192 + 64, 200))
