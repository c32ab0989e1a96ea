"""GPU: the split fan-in open (cz_open_fanin_split, k_open_fanin_tiles, k_fanin_join) against the receive model of
tests/rx_model.py.

Truth never comes from the kernels under test: bodies are sealed by the CPU oracle and damaged as rx_model damages
them, and every body's status, flags byte, payload and nonce come from rx_model.frame_status with the floor given
explicitly (the Call model of tests/test_gpu_fanin.py, whose layout -- 64 guard bytes between the runs' ranges,
three unused record entries around every run -- is reused).  cz_open_fanin_runs and cz_open_batch on equivalent
inputs are the second yardstick.  Comparison is bit-exact over whole sentinel-filled buffers: output bytes before,
between and after the runs, status and nonce entries outside the runs' record ranges.  d_work starts as 0xC3 bytes
in every call and must stay so behind its 64 * npart bytes."""
import numpy as np
import pytest

import rx_model as rx
from cz_testlib import DESC_DTYPE
from test_gpu_fanin import NKEYS, NN_SENT, SENT, ST_SENT, Body, Call, Run, _dev, _precom, _r, _valid, owns
from test_gpu_fanin import gpu  # noqa: F401  (the module-scoped device fixture: keys, subkeys, torch)

pytestmark = pytest.mark.gpu

LINES, DIRECT = 0, 1
WORK = 0xC3


class SplitCall(Call):
    def run_split(self, g, phase_in=0, phase_out=0, seg_blocks=2, plan_for=None, edit_plan=None, nonces=True):
        """open the call's runs on the grid with the buffers at the given byte phases; plan_for: the phases the
        plan is made for (default: the launch's own).  Returns (out, status, nonces, plan) as numpy arrays."""
        t = g.torch
        buf_in = t.zeros(self.in_bytes + 16, dtype=t.uint8, device=g.dev)
        buf_out = t.full((self.out_bytes + 32,), SENT, dtype=t.uint8, device=g.dev)
        d_in = buf_in[phase_in:phase_in + self.in_bytes]
        d_in.copy_(t.from_numpy(self.hin))
        d_out = buf_out[phase_out:phase_out + self.out_bytes]
        status = t.from_numpy(np.full(self.nrec, ST_SENT, dtype=np.uint16).view(np.int16)).to(g.dev)
        nn = t.from_numpy(np.full(self.nrec, NN_SENT, dtype=np.uint64).view(np.int64)).to(g.dev) if nonces else None
        pi, po = plan_for if plan_for is not None else (phase_in, phase_out)
        plan = g.batch.plan_fanin_split(self.run_rec, buf_in.data_ptr() + pi, buf_out.data_ptr() + po, seg_blocks=seg_blocks)
        if edit_plan:
            edit_plan(plan)
        plan.to(g.dev)
        work = t.full((64 * plan.npart + 64,), WORK, dtype=t.uint8, device=g.dev)
        g.batch.open_fanin_split(plan, d_in, _dev(g, self.subs), g.subkeys, d_out, status, nonces=nn, work=work,
                                 subs_np=self.subs)
        t.cuda.synchronize()
        whole = buf_out.cpu().numpy()
        assert (whole[:phase_out] == SENT).all() and (whole[phase_out + self.out_bytes:] == SENT).all()
        assert (work[64 * plan.npart:].cpu().numpy() == WORK).all(), "d_work written past its 64 * npart bytes"
        return (whole[phase_out:phase_out + self.out_bytes], status.cpu().numpy().view(np.uint16),
                nn.cpu().numpy().view(np.uint64) if nonces else None, plan)

    def same_as_runs(self, g, got, what):
        """whole buffers against cz_open_fanin_runs on the same runs and records"""
        out, st, nn, _ = self.run(g)
        assert np.array_equal(got[1], st), f"{what}: statuses differ from cz_open_fanin_runs'"
        assert got[2] is None or np.array_equal(got[2], nn), f"{what}: nonces differ from cz_open_fanin_runs'"
        bad = np.nonzero(got[0] != out)[0]
        assert not len(bad), f"{what}: output byte {bad[0]} differs from cz_open_fanin_runs' ({self.where_out(int(bad[0]))})"


def _strides(size, in_kind, out_kind):
    nout = max(size - 33, 0)
    in_stride = (size, _r(size, 16), _r(size, 128))[in_kind]
    big16 = _r(nout, 16) + 272
    out_stride = (_r(max(nout, 1), 128), nout if nout else 64, big16 + 16 if big16 % 128 == 0 else big16)[out_kind]
    return in_stride, out_stride


# ---- one mixed call at seg_blocks 2 -----------------------------------------------------------------------
SIZES = (33, 34, 96, 97, 129, 161, 225, 4129)       # 1, 1, 2, 2, 3, 3, 4 and 65 blocks: whole up to 3 at seg_blocks 2
COUNTS = (1, 63, 64, 65, 130)


@pytest.fixture(scope="module")
def mixed():
    """every size x input stride x output stride, counts and key arrangements cycling: with a key per body every
    body is a connection of its own above a plain floor; with three keys shared by all, body j belongs to
    connection j % 3 and takes body j - 3 of its run as floor (the same wave, or the wave before)"""
    runs, k = [], 0
    for size in SIZES:
        for out_kind in range(3):
            for in_kind in range(3):
                in_stride, out_stride = _strides(size, in_kind, out_kind)
                count = COUNTS[k % len(COUNTS)]
                per_body = (k // 2) % 2 == 0
                bodies = []
                for j in range(count):
                    key = (j * 5 + k) % NKEYS if per_body else j % 3
                    nonce = 1000 * k + 10 + 2 * j
                    data = _valid(size, nonce, key, 91000 + 300 * k + j, flags=j & 3)
                    if per_body or j < 3:
                        # (every 11th body of a connection of its own is a replay: floor = its nonce)
                        floor = ("plain", nonce if per_body and j % 11 == 5 else nonce - 1 - (j % 2))
                    else:
                        floor = ("run", len(runs), j - 3)
                    bodies.append(Body(data, key, floor))
                runs.append(Run(size, in_stride, out_stride, bodies))
                k += 1
    call = SplitCall(runs)
    assert {owns(r.out_stride) for r in runs} == {True, False}
    return call


@pytest.mark.parametrize("phase", [0, 8, 1])
def test_mixed_call(gpu, mixed, phase):
    got = mixed.run_split(gpu, phase, phase)
    plan = got[3]
    split = [r for r in mixed.runs if r.size > 3 * 64]
    waves = lambda rs: sum((len(r.bodies) + 63) // 64 for r in rs)      # noqa: E731
    segs = lambda r: 1 if r.size <= 192 else (((r.size + 63) // 64 - 1) + 1) // 2   # noqa: E731
    assert sum(plan.class_count) == len(plan.tiles) == sum(segs(r) * waves([r]) for r in mixed.runs)
    assert len(plan.joins) == waves(split) and plan.npart == sum(len(r.bodies) * segs(r) for r in split)
    if phase == 0:
        assert all(plan.class_count), plan.class_count              # both launches and the join
    else:
        assert plan.class_count[LINES] == 0
    assert {rx.ST_OK, rx.ST_SEQUENCE} <= set(mixed.statuses)
    mixed.check(got, f"phase {phase}")
    if phase == 0:
        mixed.same_as_runs(gpu, got, "mixed call")


def test_without_nonces(gpu, mixed):
    mixed.check(mixed.run_split(gpu, nonces=False), "d_nonces null")


# ---- seg_blocks 1 -------------------------------------------------------------------------------------------
def test_seg_blocks_1(gpu):
    """bodies of 1, 2, 3 and 5 blocks: whole, whole (one segment by the count), [0, 2) + one block, and four tiles"""
    runs = []
    for k, size in enumerate((40, 100, 161, 300)):
        for count, in_kind, out_kind in ((65, 2, 0), (3, 0, 1)):
            in_stride, out_stride = _strides(size, in_kind, out_kind)
            # (every seventh body replays its floor)
            bodies = [Body(_valid(size, 50 + j, j % NKEYS, 600 + 70 * k + j, flags=j & 3), j % NKEYS,
                           ("plain", 49 + j + (j % 7 == 3))) for j in range(count)]
            runs.append(Run(size, in_stride, out_stride, bodies))
    call = SplitCall(runs)
    got = call.run_split(gpu, seg_blocks=1)
    plan = got[3]
    cuts = {}
    for t in plan.tiles.tolist():
        cuts.setdefault((t[0], t[1]), []).append((t[2], t[3]))
    assert sorted(cuts[(0, 0)]) == [(0, 1)] and sorted(cuts[(2, 64)]) == [(0, 2)]
    assert sorted(cuts[(4, 0)]) == [(0, 2), (2, 1)] and sorted(cuts[(7, 0)]) == [(0, 2), (2, 1), (3, 1), (4, 1)]
    assert rx.ST_SEQUENCE in call.statuses
    call.check(got, "seg_blocks 1")
    call.same_as_runs(gpu, got, "seg_blocks 1")


# ---- long bodies --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_call():
    """64 KiB payloads of 130 connections, two bodies damaged in a late segment and in the tag"""
    size, bodies = 65569, []
    for j in range(130):
        data = bytearray(_valid(size, 7 + j, j % NKEYS, 4000 + j, flags=j & 3))
        if j == 66:
            data[60000] ^= 4
        if j == 129:
            data[20] ^= 1
        bodies.append(Body(bytes(data), j % NKEYS, ("plain", 6 + j)))
    return SplitCall([Run(size, _r(size, 128), 65536, bodies)])


@pytest.mark.parametrize("seg_blocks", [8, 0])
def test_long_bodies(gpu, long_call, seg_blocks):
    got = long_call.run_split(gpu, seg_blocks=seg_blocks)
    plan = got[3]
    seg = seg_blocks or 4                     # (8.5 MB in all: flush_in's shortest length)
    assert int(plan.tiles["nseg"][0]) == 1024 // seg and len(plan.tiles) == 3 * (1024 // seg)
    last = max(plan.tiles.tolist(), key=lambda t: t[2])
    assert last[2] == 1025 - seg and last[3] == seg      # the last segment ends with the 33-byte block
    assert long_call.statuses.count(rx.ST_CRYPTO) == 2
    long_call.check(got, f"seg_blocks {seg_blocks}")


# ---- faults -------------------------------------------------------------------------------------------------
FAULT_AT = (0, 37, 63, 67)      # lanes 0, 37 and 63 of the full wave, lane 3 of the 6-lane partial wave
KINDS = ("tag", "ct_last", "ct_middle", "name3", "name7", "wrong_dir", "replay", "replay_tag", "flags_ff")


def _fault_body(kind, nonce, key, seed, size=4129):
    if kind == "ct_middle":     # one ciphertext byte inside the third of the 16 segments only (blocks 9..12)
        data = bytearray(_valid(size, nonce, key, seed))
        data[64 * 10 + 5] ^= 0x10
        return bytes(data)
    return rx.build_body(rx.Frame(nonce, size, kind, 1, seed), rx.SERVER, _precom(key))


@pytest.fixture(scope="module")
def faults():
    runs = []
    for k, kind in enumerate(KINDS):
        bodies = []
        for j in range(70):
            nonce, key = 100 * k + 2 * j + 5, (j + k) % NKEYS
            bad = j in FAULT_AT
            data = _fault_body(kind, nonce, key, 8000 + 100 * k + j) if bad else _valid(4129, nonce, key, 8000 + 100 * k + j, flags=j & 3)
            floor = nonce if bad and kind in ("replay", "replay_tag") else nonce - 1
            bodies.append(Body(data, key, ("plain", floor)))
        runs.append(Run(4129, 4224, 4096 if k % 2 == 0 else 4103, bodies))
    # bodies cut to 32 bytes: the whole run is MALFORMED, only owned slots' zeros are written
    for out_stride in (128, 300):
        bodies = [Body(_valid(97, 9 + j, 0, 8900 + j)[:32], 0, ("plain", 3)) for j in range(70)]
        runs.append(Run(32, 32, out_stride, bodies))
    call = SplitCall(runs)
    want = {"tag": rx.ST_CRYPTO, "ct_last": rx.ST_CRYPTO, "ct_middle": rx.ST_CRYPTO, "name3": rx.ST_COMMAND,
            "name7": rx.ST_OK, "wrong_dir": rx.ST_CRYPTO, "replay": rx.ST_SEQUENCE, "replay_tag": rx.ST_SEQUENCE,
            "flags_ff": rx.ST_OK}
    for k, kind in enumerate(KINDS):
        st = call.statuses[70 * k:70 * k + 70]
        assert [st[j] for j in FAULT_AT] == [want[kind]] * 4 and sum(s != rx.ST_OK for s in st) in (0, 4), kind
    assert call.statuses[70 * len(KINDS):] == [rx.ST_MALFORMED] * 140
    return call


@pytest.mark.parametrize("phase", [0, 8])
def test_faults(gpu, faults, phase):
    got = faults.run_split(gpu, phase, phase, seg_blocks=4)
    assert int(got[3].tiles["nseg"][0]) == 16
    faults.check(got, f"faults, phase {phase}")
    # flags byte 0xff: all 8 bits reach the status word
    k = KINDS.index("flags_ff")
    assert got[1][faults.first[k] + 37] == 0xff00
    if phase == 0:
        faults.same_as_runs(gpu, got, "faults")


# ---- chains -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chains():
    size = 4129
    ext, runs = [], []
    # run 0: four connections interleaved, 130 bodies: floors name a body of the same wave, bodies 64..67 one of
    # the wave before; run 1 continues the connections: its floors name bodies of run 0.  Floors 2^32 - 5,
    # 2^63 + 7, 2^64 - 50: the chains cross 2^32 and wrap.  Connection 1's body 9 is rejected by its tag and is
    # still the floor of body 13.
    nonce = {c: (0, (1 << 32) - 5, (1 << 63) + 7, (1 << 64) - 50)[c] for c in range(4)}
    last = {}
    for ri, (count, in_stride, out_stride) in enumerate(((130, 4224, 4096), (70, size, 4103))):
        bodies = []
        for j in range(count):
            c = j % 4
            floor = ("run",) + last[c] if c in last else ("plain", nonce[c])
            nonce[c] = (nonce[c] + 1 + (j % 3)) & rx.M64
            data = bytearray(_valid(size, nonce[c], c, 5000 + 200 * ri + j, flags=j & 1))
            if (ri, j) == (0, 9):
                data[16] ^= 1
            if (ri, j) == (0, 70):
                data[3] ^= 0x20                                   # a floor that was rejected as a COMMAND
            bodies.append(Body(bytes(data), c, floor))
            last[c] = (ri, j)
        runs.append(Run(size, in_stride, out_stride, bodies))
    # run 2: connections whose previous body is in no run -- it lies elsewhere in d_in, of another size; accepted
    # or not, its wire nonce is the floor
    bodies = []
    for j in range(66):
        n_prev = 500 + 3 * j
        prev = bytearray(_valid(40 + (j % 5), n_prev, 4, 6000 + j))
        if j % 4 == 1:
            prev[16] ^= 1
        ext.append(Body(bytes(prev), 4, ("plain", 0)))
        n = n_prev + (0 if j % 6 == 2 else 1)                      # every sixth replays the previous body's nonce
        bodies.append(Body(_valid(size, n, 4, 6100 + j), 4, ("ext", j)))
    runs.append(Run(size, 4144, 4112, bodies))
    # run 3: records without CHECK_NONCE: a replay of the floor and a nonce below it are accepted
    bodies = [Body(_valid(225, 50, 5, 7100), 5, ("plain", 50), check=False)]
    bodies.append(Body(_valid(225, 49, 5, 7101), 5, ("run", 3, 0), check=False))
    bodies.append(Body(_valid(225, 49, 5, 7102), 5, ("run", 3, 1), check=True))
    runs.append(Run(225, 225, 192, bodies))
    call = SplitCall(runs, ext)
    assert call.statuses[-3:] == [rx.ST_OK, rx.ST_OK, rx.ST_SEQUENCE]
    assert any(o % 16 == 8 for o in call.ext_off) and all(o % 8 == 0 for o in call.ext_off)
    assert {rx.ST_OK, rx.ST_SEQUENCE, rx.ST_CRYPTO, rx.ST_COMMAND} <= set(call.statuses)
    return call


@pytest.mark.parametrize("phase", [0, 8, 1])
def test_chains(gpu, chains, phase):
    got = chains.run_split(gpu, phase, phase, seg_blocks=4)
    chains.check(got, f"phase {phase}")
    if phase == 0:
        chains.same_as_runs(gpu, got, "chains")


# ---- the class is never a correctness choice ----------------------------------------------------------------
def _all_lines(plan):
    plan.class_count = [len(plan.tiles), 0]


def _all_direct(plan):
    plan.class_count = [0, len(plan.tiles)]


def _reversed(plan):
    plan.tiles = np.ascontiguousarray(plan.tiles[::-1])


@pytest.mark.parametrize("edit", [_all_lines, _all_direct, _reversed])
def test_forced_tables(gpu, mixed, faults, edit):
    """the same runs with every tile handed to the line slice (partial waves, unaligned runs and waves with a
    rejected lane open lane-wise there), every tile handed to the lane-wise slice, and the planner's table in
    reversed order under the same class counts"""
    mixed.check(mixed.run_split(gpu, edit_plan=edit), edit.__name__)
    faults.check(faults.run_split(gpu, seg_blocks=4, edit_plan=edit), edit.__name__ + ", faults")


@pytest.mark.parametrize("shift", [8, 1])
def test_plan_for_other_addresses(gpu, mixed, shift):
    """a plan made for 16-byte aligned buffers, launched on buffers shifted by 8 bytes and by 1 byte: the waves ride
    in the line slice and open lane-wise -- the same output"""
    got = mixed.run_split(gpu, shift, shift, plan_for=(0, 0))
    assert got[3].class_count[LINES]
    mixed.check(got, f"planned for phase 0, run at {shift}")


def test_caller_built_tables(gpu, chains):
    """tables under the header's rule: every (run, 64 bodies) cut at points of the caller's own -- one or more
    blocks each, tiles after the first from block 2 on -- in shuffled order"""
    def recut(plan):
        rng = np.random.default_rng(5)
        tiles, joins, part = [], [], 0
        for ri, r in enumerate(chains.runs):
            nblk = (r.size + 63) // 64
            for first in range(0, len(r.bodies), 64):
                inner = sorted(rng.choice(np.arange(2, nblk), size=min(int(rng.integers(1, 9)), nblk - 2), replace=False).tolist())
                edges = [0] + inner + [nblk]
                nseg, lanes = len(edges) - 1, min(64, len(r.bodies) - first)
                joins.append((ri, first, part, nseg))
                tiles += [(ri, first, edges[s], edges[s + 1] - edges[s], part + s, nseg) for s in range(nseg)]
                part += lanes * nseg
        order = rng.permutation(len(tiles))
        plan.tiles = np.array([tiles[i] for i in order], dtype=plan.tiles.dtype)
        plan.joins = np.array(joins, dtype=plan.joins.dtype)
        plan.npart, plan.class_count = part, [len(tiles) // 2, len(tiles) - len(tiles) // 2]
    chains.check(chains.run_split(gpu, edit_plan=recut), "caller-built tables")


# ---- equivalence and capture --------------------------------------------------------------------------------
def test_same_as_open_batch(gpu, chains):
    """the same bodies through cz_open_batch, one descriptor per body (the ext bodies first), FLOOR_IS_BODY records
    as prev chains: equal statuses and nonces, equal payload bytes of every frame that was decrypted"""
    g, call = gpu, chains
    index, rows = {}, []
    for k, b in enumerate(call.ext):
        index[("ext", k)] = len(rows)
        rows.append((call.ext_off[k], 0, len(b.data), b.from_srv * NKEYS + b.key, 0, 0, -1))
    for ri, r in enumerate(call.runs):
        for j, b in enumerate(r.bodies):
            index[("run", ri, j)] = len(rows)
            plain = b.floor[0] == "plain"
            rows.append((call.in_off[ri] + j * r.in_stride, call.out_off[ri] + j * r.out_stride, r.size,
                         b.from_srv * NKEYS + b.key, b.floor[1] & rx.M64 if plain else 0, 0x100 if b.check else 0,
                         -1 if plain else index[tuple(b.floor)]))
    desc = np.array(rows, dtype=DESC_DTYPE)
    scratch = call.out_bytes
    for k in range(len(call.ext)):
        desc["out_off"][k] = scratch
        scratch += 64
    t = g.torch
    d_out = t.full((scratch + 64,), SENT, dtype=t.uint8, device=g.dev)
    status = t.full((len(desc),), -1, dtype=t.int16, device=g.dev)
    nonces = t.zeros(len(desc), dtype=t.int64, device=g.dev)
    g.batch.open_batch(_dev(g, desc), len(desc), _dev(g, call.hin), d_out, g.subkeys, status, nonces=nonces, desc_np=desc)
    t.cuda.synchronize()
    out, st, nn, _ = call.run_split(g, seg_blocks=4)
    b_out, b_st, b_nn = d_out.cpu().numpy(), status.cpu().numpy().view(np.uint16), nonces.cpu().numpy().view(np.uint64)
    for ri, r in enumerate(call.runs):
        nout = max(r.size - 33, 0)
        for j in range(len(r.bodies)):
            d, rec = index[("run", ri, j)], call.first[ri] + j
            assert st[rec] == b_st[d] and nn[rec] == b_nn[d], call.where(rec)
            if (st[rec] & 0xff) in (rx.ST_OK, rx.ST_CRYPTO):
                o = call.out_off[ri] + j * r.out_stride
                assert out[o:o + nout].tobytes() == b_out[o:o + nout].tobytes(), call.where(rec)


def test_empty_calls(gpu):
    """no runs, and runs without bodies: CZ_OK, nothing launched, nothing written"""
    g, t = gpu, gpu.torch
    for runs in (np.zeros(0, dtype=g.batch.FANIN_RUN_DTYPE), np.zeros(2, dtype=g.batch.FANIN_RUN_DTYPE)):
        buf = t.full((256,), SENT, dtype=t.uint8, device=g.dev)
        st = t.full((4,), 0x5A5A, dtype=t.int16, device=g.dev)
        plan = g.batch.plan_fanin_split(runs, buf, buf).to(g.dev)
        assert len(plan.tiles) == 0 and plan.npart == 0
        g.batch.open_fanin_split(plan, buf, _dev(g, np.zeros(1, dtype=g.batch.FANIN_SUB_DTYPE)), g.subkeys, buf, st)
        t.cuda.synchronize()
        assert (buf.cpu().numpy() == SENT).all() and (st.cpu().numpy() == 0x5A5A).all()
