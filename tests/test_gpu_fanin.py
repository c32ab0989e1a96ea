"""GPU: the fan-in open (cz_open_fanin_runs, k_open_fanin_runs) against the receive model of tests/rx_model.py.

Truth never comes from the kernel under test: bodies are sealed by the CPU oracle and damaged as the scenario
table damages them, and every body's status, flags byte, payload and nonce come from rx_model.frame_status with
the floor given explicitly (a FLOOR_IS_BODY record's floor is the wire nonce of the body it names, accepted or
not: rx_model.chain_expect's rule).  cz_open_batch on equivalent descriptors is the second yardstick.  Whole
sentinel-filled buffers are compared: output bytes before, between and after the runs, owned slots past their
payloads, rejected frames' slots, and status and nonce entries outside the runs' record ranges."""
import numpy as np
import pytest

import rx_model as rx
from cz_testlib import DESC_DTYPE, splitmix_bytes

pytestmark = pytest.mark.gpu

SENT = 0xA5          # output bytes before a call
ST_SENT = 0x5A5A     # status entries before a call
NN_SENT = 0x7E7E7E7E7E7E7E7E
GUARD = 64           # bytes between two runs' ranges, entries between two runs' record ranges: 3
NKEYS = 7
LINES, REGION, DIRECT = 0, 1, 2
CHECK, IS_BODY = 1, 2


def _r(n, a):
    return (n + a - 1) // a * a


def _precom(k):
    return rx.PRECOM if k == 0 else splitmix_bytes(32, 0xF00D + k)


def owns(stride):
    """the output-ownership rule of cz_open_uniform, by the stride alone (restated from the header)"""
    return (stride % 128 == 0 and stride < (1 << 25)) or (stride % 16 == 0 and stride <= 256)


class _Gpu:
    pass


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from jeromq_amd import _lib, batch
    g = _Gpu()
    g.torch, g.dev, g.L, g.batch = torch, torch.device("cuda:0"), _lib, batch
    k = torch.tensor([list(_precom(i)) for i in range(NKEYS)], dtype=torch.uint8, device=g.dev)
    # key index = from_server * NKEYS + k
    g.subkeys = torch.cat([batch.subkeys(k, _lib.CZ_DIR_C2S), batch.subkeys(k, _lib.CZ_DIR_S2C)])
    return g


def _dev(g, a):
    return g.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(g.dev)


# ---- a call's description -----------------------------------------------------------------------------
class Body:
    """One body: its bytes, the key it is opened under, and its floor -- ("plain", value), ("run", r, j): the
    body j of run r, or ("ext", k): the k-th body that lies in d_in outside every run."""

    def __init__(self, data, key, floor, check=True, from_srv=0):
        self.data, self.key, self.floor, self.check, self.from_srv = bytes(data), key, floor, check, from_srv


class Run:
    def __init__(self, size, in_stride, out_stride, bodies):
        self.size, self.in_stride, self.out_stride, self.bodies = size, in_stride, out_stride, bodies
        assert all(len(b.data) == size for b in bodies)


class Call:
    """Runs laid out in d_in / d_out with GUARD bytes between their ranges (run offsets are multiples of 128,
    so the base phase and the strides alone decide a run's alignment class), `ext` bodies behind them, the
    records with three unused entries before, between and after the runs' ranges -- and what the model says
    every buffer holds afterwards."""

    def __init__(self, runs, ext=()):
        self.runs, self.ext = runs, list(ext)
        io, oo, rec = 128, 128, 3
        self.in_off, self.out_off, self.first = [], [], []
        for r in runs:
            n, nout = len(r.bodies), max(r.size - 33, 0)
            self.in_off.append(io)
            self.out_off.append(oo)
            self.first.append(rec)
            io = _r(io + (n - 1) * r.in_stride + r.size + GUARD, 128) if n else io
            span = n * r.out_stride if owns(r.out_stride) else (n - 1) * r.out_stride + nout
            oo = _r(oo + span + GUARD, 128) if n else oo
            rec += n + 3
        self.ext_off = []
        for b in self.ext:
            self.ext_off.append(io)
            io = _r(io + len(b.data) + 8, 8) + 8          # 8-byte aligned, not all 16-byte aligned
        self.in_bytes, self.out_bytes, self.nrec = io + 64, oo + 64, rec
        self.hin = np.zeros(self.in_bytes, dtype=np.uint8)
        for ri, r in enumerate(runs):
            for j, b in enumerate(r.bodies):
                o = self.in_off[ri] + j * r.in_stride
                self.hin[o:o + r.size] = np.frombuffer(b.data, dtype=np.uint8)
        for k, b in enumerate(self.ext):
            self.hin[self.ext_off[k]:self.ext_off[k] + len(b.data)] = np.frombuffer(b.data, dtype=np.uint8)
        self._model()

    def body_off(self, ref):
        if ref[0] == "run":
            return self.in_off[ref[1]] + ref[2] * self.runs[ref[1]].in_stride
        return self.ext_off[ref[1]]

    def body_of(self, ref):
        return self.runs[ref[1]].bodies[ref[2]] if ref[0] == "run" else self.ext[ref[1]]

    def _model(self):
        from jeromq_amd import batch
        self.run_rec = np.zeros(len(self.runs), dtype=batch.FANIN_RUN_DTYPE)
        self.subs = np.zeros(self.nrec, dtype=batch.FANIN_SUB_DTYPE)
        self.subs["floor"], self.subs["key_idx"], self.subs["flags"] = 0xDEAD0000DEAD, 0x7FFFFFF0, 1   # never read
        self.want_out = np.full(self.out_bytes, SENT, dtype=np.uint8)
        self.want_st = np.full(self.nrec, ST_SENT, dtype=np.uint16)
        self.want_nn = np.full(self.nrec, NN_SENT, dtype=np.uint64)
        self.statuses = []
        for ri, r in enumerate(self.runs):
            nout = max(r.size - 33, 0)
            self.run_rec[ri] = (self.in_off[ri], r.in_stride, self.out_off[ri], r.out_stride, r.size, self.first[ri],
                                len(r.bodies), 0)
            for j, b in enumerate(r.bodies):
                rec = self.first[ri] + j
                if b.floor[0] == "plain":
                    floor, word = b.floor[1] & rx.M64, b.floor[1] & rx.M64
                    fl = CHECK if b.check else 0
                else:
                    floor, word = rx.wire_nonce(self.body_of(b.floor).data), self.body_off(b.floor)
                    fl = (CHECK if b.check else 0) | IS_BODY
                self.subs[rec] = (word, b.from_srv * NKEYS + b.key, fl)
                st, flags, payload, nonce = rx.frame_status(b.data, floor, b.check, b.from_srv, _precom(b.key))
                self.statuses.append(st)
                self.want_st[rec] = st | ((flags << 8) if st == rx.ST_OK else 0)
                self.want_nn[rec] = nonce if nonce is not None else 0
                o = self.out_off[ri] + j * r.out_stride
                if owns(r.out_stride):
                    self.want_out[o:o + r.out_stride] = 0              # zeros past a payload, rejected slots whole
                if st == rx.ST_OK:
                    self.want_out[o:o + nout] = np.frombuffer(payload, dtype=np.uint8)
                else:
                    self.want_out[o:o + nout] = 0                      # a rejected frame's payload bytes

    def run(self, g, phase_in=0, phase_out=0, plan_for=None, edit_plan=None, nonces=True):
        """open the call's runs with the buffers at the given byte phases; plan_for: the phases the plan is made
        for (default: the launch's own).  Returns (out, status, nonces, plan) as numpy arrays."""
        t = g.torch
        buf_in = t.zeros(self.in_bytes + 16, dtype=t.uint8, device=g.dev)
        buf_out = t.full((self.out_bytes + 32,), SENT, dtype=t.uint8, device=g.dev)
        d_in = buf_in[phase_in:phase_in + self.in_bytes]
        d_in.copy_(t.from_numpy(self.hin))
        d_out = buf_out[phase_out:phase_out + self.out_bytes]
        status = t.from_numpy(np.full(self.nrec, ST_SENT, dtype=np.uint16).view(np.int16)).to(g.dev)
        nn = t.from_numpy(np.full(self.nrec, NN_SENT, dtype=np.uint64).view(np.int64)).to(g.dev) if nonces else None
        pi, po = plan_for if plan_for is not None else (phase_in, phase_out)
        plan = g.batch.plan_fanin(self.run_rec, buf_in.data_ptr() + pi, buf_out.data_ptr() + po)
        if edit_plan:
            edit_plan(plan)
        plan.to(g.dev)
        g.batch.open_fanin_runs(plan, d_in, _dev(g, self.subs), g.subkeys, d_out, status, nonces=nn, subs_np=self.subs)
        t.cuda.synchronize()
        whole = buf_out.cpu().numpy()
        assert (whole[:phase_out] == SENT).all() and (whole[phase_out + self.out_bytes:] == SENT).all()
        return (whole[phase_out:phase_out + self.out_bytes], status.cpu().numpy().view(np.uint16),
                nn.cpu().numpy().view(np.uint64) if nonces else None, plan)

    def check(self, got, what):
        out, st, nn, _plan = got
        bad_st = np.nonzero(st != self.want_st)[0]
        assert not len(bad_st), f"{what}: status[{bad_st[0]}] = {st[bad_st[0]]:#x}, model {self.want_st[bad_st[0]]:#x}" \
                                f" ({len(bad_st)} differ; {self.where(int(bad_st[0]))})"
        if nn is not None:
            bad_nn = np.nonzero(nn != self.want_nn)[0]
            assert not len(bad_nn), f"{what}: nonce[{bad_nn[0]}] = {int(nn[bad_nn[0]]):#x}, model " \
                                    f"{int(self.want_nn[bad_nn[0]]):#x} ({self.where(int(bad_nn[0]))})"
        bad = np.nonzero(out != self.want_out)[0]
        assert not len(bad), f"{what}: output byte {bad[0]} = {out[bad[0]]:#x}, model {self.want_out[bad[0]]:#x} " \
                             f"({len(bad)} differ; {self.where_out(int(bad[0]))})"

    def where(self, rec):
        for ri, r in enumerate(self.runs):
            if self.first[ri] <= rec < self.first[ri] + len(r.bodies):
                return f"run {ri} body {rec - self.first[ri]}: size {r.size}, strides {r.in_stride} / {r.out_stride}"
        return "outside every run"

    def where_out(self, o):
        for ri in reversed(range(len(self.runs))):
            if o >= self.out_off[ri]:
                r = self.runs[ri]
                j = (o - self.out_off[ri]) // r.out_stride if r.out_stride else 0
                return f"run {ri} (size {r.size}, strides {r.in_stride} / {r.out_stride}, {len(r.bodies)} bodies), slot {j}"
        return "before the first run"


def _valid(size, nonce, key, seed, flags=0):
    return rx.build_body(rx.Frame(nonce, size, None, flags, seed), rx.SERVER, _precom(key))


# ---- the mixed call -------------------------------------------------------------------------------------
SIZES = (33, 34, 96, 97, 161, 288, 289, 4129)      # 288 / 289: nout 255 / 256, the line-class edge
COUNTS = (1, 63, 64, 65, 130, 257)


@pytest.fixture(scope="module")
def mixed():
    """every size x out stride x in stride, counts and key arrangements cycling: with a key per body every body
    is a connection of its own above a plain floor; with three keys shared by all, body j belongs to connection
    j % 3 and takes body j - 3 of its run as floor (the same wave, or the wave before)"""
    runs, k = [], 0
    for size in SIZES:
        nout = size - 33
        for os_kind in range(4):
            for is_kind in range(2):
                out_stride = (_r(nout, 128), _r(nout, 128) + 128, nout, nout + 7)[os_kind]
                in_stride = (_r(size, 128), size)[is_kind]
                count = COUNTS[k % len(COUNTS)]
                per_body = (k // 2) % 2 == 0
                bodies = []
                for j in range(count):
                    key = (j * 5 + k) % NKEYS if per_body else j % 3
                    nonce = 1000 * k + 10 + 2 * j
                    data = _valid(size, nonce, key, 77000 + 300 * k + j, flags=j & 3)
                    if per_body or j < 3:
                        # (every 11th body of a connection of its own is a replay: floor = its nonce)
                        floor = ("plain", nonce if per_body and j % 11 == 5 else nonce - 1 - (j % 2))
                    else:
                        floor = ("run", len(runs), j - 3)
                    bodies.append(Body(data, key, floor))
                runs.append(Run(size, in_stride, out_stride, bodies))
                k += 1
    return Call(runs)


@pytest.mark.parametrize("phase_in,phase_out", [(0, 0), (8, 8), (1, 1), (0, 8), (8, 0)])
def test_mixed_call(gpu, mixed, phase_in, phase_out):
    got = mixed.run(gpu, phase_in, phase_out)
    plan = got[3]
    assert sum(plan.class_count) == plan.nwaves == sum((len(r.bodies) + 63) // 64 for r in mixed.runs)
    if (phase_in, phase_out) == (0, 0):
        assert all(plan.class_count), plan.class_count            # one call, every class
    else:
        assert plan.class_count[LINES] == plan.class_count[REGION] == 0
    assert {rx.ST_OK, rx.ST_SEQUENCE} <= set(mixed.statuses)
    mixed.check(got, f"phases {phase_in}/{phase_out}")


def test_without_nonces(gpu, mixed):
    mixed.check(mixed.run(gpu, nonces=False), "d_nonces null")


# ---- chains ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chains():
    size = 133
    ext, runs = [], []
    # run 0: four connections interleaved, 130 bodies; run 1 (another size class: lane-wise) continues them:
    # its floors name bodies of run 0.  Nonces climb by 1..3 per connection.
    nonce = {c: (0, (1 << 32) - 40, (1 << 63) - 30, (1 << 64) - 60)[c] for c in range(4)}
    last = {}
    for ri, (count, in_stride, out_stride) in enumerate(((130, 256, 128), (70, size, 107))):
        bodies = []
        for j in range(count):
            c = j % 4
            floor = ("run",) + last[c] if c in last else ("plain", nonce[c])
            nonce[c] = (nonce[c] + 1 + (j % 3)) & rx.M64
            bodies.append(Body(_valid(size, nonce[c], c, 5000 + 200 * ri + j, flags=j & 1), c, floor))
            last[c] = (ri, j)
        runs.append(Run(size, in_stride, out_stride, bodies))
    # run 2: connections whose previous body is in no run -- it lies elsewhere in d_in, of another size, at 8-byte
    # and 16-byte aligned offsets; accepted or not, its wire nonce is the floor
    bodies = []
    for j in range(66):
        n_prev = 500 + 3 * j
        prev = bytearray(_valid(40 + (j % 5), n_prev, 4, 6000 + j))
        if j % 4 == 1:
            prev[16] ^= 1                                   # a previous body that was rejected by its tag
        ext.append(Body(bytes(prev), 4, ("plain", 0)))
        n = n_prev + (0 if j % 6 == 2 else 1)               # every sixth replays the previous body's nonce
        bodies.append(Body(_valid(size, n, 4, 6100 + j), 4, ("ext", j)))
    runs.append(Run(size, 144, 112, bodies))
    # run 3: the nonce runs of the table, each a connection of its own under its own key: negative longs, the
    # wrap, crossing 2^32 and 2^63; the model's statuses must be the table's
    bodies, table = [], []
    for k, (name, (floor, nonces, sts)) in enumerate(rx.NONCE_RUNS.items()):
        for i, n in enumerate(nonces):
            fl = ("plain", floor) if i == 0 else ("run", 3, len(bodies) - 1)
            bodies.append(Body(_valid(97, n, k, 7000 + 10 * k + i), k, fl))
            table.append(sts[i])
    # ... and records without CHECK_NONCE: a replay of the floor and a nonce below it are accepted
    bodies.append(Body(_valid(97, 50, 5, 7100), 5, ("plain", 50), check=False))
    bodies.append(Body(_valid(97, 49, 5, 7101), 5, ("run", 3, len(bodies) - 1), check=False))
    bodies.append(Body(_valid(97, 49, 5, 7102), 5, ("run", 3, len(bodies) - 1), check=True))
    table += [rx.ST_OK, rx.ST_OK, rx.ST_SEQUENCE]
    runs.append(Run(97, 97, 64, bodies))
    call = Call(runs, ext)
    assert call.statuses[-len(table):] == table
    return call


@pytest.mark.parametrize("phase", [0, 8, 1])
def test_chains(gpu, chains, phase):
    got = chains.run(gpu, phase, phase)
    if phase == 0:
        assert got[3].class_count[REGION] >= 3          # run 0's full waves and run 2's are staged
    assert {rx.ST_OK, rx.ST_SEQUENCE} <= set(chains.statuses)
    chains.check(got, f"phase {phase}")


# ---- faults ---------------------------------------------------------------------------------------------
def _fault_call(role, layout):
    """the uniform chains of the scenario table (sizes 34, 161 and 4129, 130 bodies, UNIFORM_KINDS rotated over
    bodies 0, 1, 63, 64, 65 and the last, nonces from NONCE_RUNS), one run and one connection each: body 0 above
    the scenario's floor, body i above body i - 1's wire nonce, rejected or not"""
    runs, expect = [], []
    fs = rx.from_server(role)
    for sc in rx.scenarios():
        if not sc.uniform or len(sc.frames) != 130:
            continue
        size, nout = sc.uniform, sc.uniform - 33
        in_stride, out_stride = {"staged": (_r(size, 128), _r(nout, 128)), "lane_wise": (size, _r(nout, 128)),
                                 "packed": (_r(size, 16), nout + 7)}[layout]
        ri = len(runs)
        bodies = [Body(b, 0, ("plain", sc.floor) if i == 0 else ("run", ri, i - 1), from_srv=fs)
                  for i, b in enumerate(sc.bodies(role))]
        runs.append(Run(size, in_stride, out_stride, bodies))
        expect += [e[0] for e in sc.raw_expect(role)]
    call = Call(runs)
    assert call.statuses == expect                    # the explicit-floor model agrees with chain_expect
    assert {rx.ST_OK, rx.ST_CRYPTO, rx.ST_COMMAND, rx.ST_SEQUENCE} <= set(expect)
    return call


@pytest.mark.parametrize("role", rx.ROLES)
@pytest.mark.parametrize("layout", ["staged", "lane_wise", "packed"])
def test_faults(gpu, role, layout):
    call = _fault_call(role, layout)
    got = call.run(gpu)
    cc = got[3].class_count
    if layout == "staged":
        assert cc[LINES] and cc[REGION]               # faults at lanes 0, 1, 63 of staged waves, 65 / last lane-wise
    else:
        assert cc[LINES] == cc[REGION] == 0
    call.check(got, f"{role} {layout}")


# ---- a table for other addresses ------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [8, 1])
def test_plan_for_other_addresses(gpu, mixed, shift):
    """a plan made for 16-byte aligned buffers, launched on buffers shifted by 8 bytes and by 1 byte: the waves
    ride in the staged classes' launches and open lane-wise -- the same output"""
    got = mixed.run(gpu, shift, shift, plan_for=(0, 0))
    assert all(got[3].class_count)
    mixed.check(got, f"planned for phase 0, run at {shift}")


def test_reversed_wave_table(gpu, mixed, chains):
    """a hand-built table, the planner's in reversed order under the same class counts: most waves ride in another
    class's launch and re-check their own run"""
    def reverse(plan):
        plan.waves = np.ascontiguousarray(plan.waves[::-1])
    for call in (mixed, chains):
        got = call.run(gpu, edit_plan=reverse)
        call.check(got, "reversed table")


# ---- equivalence ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["mixed", "chains"])
def test_same_as_open_batch(gpu, mixed, chains, which):
    """the same bodies through cz_open_batch, one descriptor per body (the ext bodies first), FLOOR_IS_BODY
    records as prev chains: equal statuses and nonces, equal payload bytes of every frame that was decrypted
    (cz_open_batch leaves the payload of a frame rejected before decryption as it was)"""
    g, call = gpu, {"mixed": mixed, "chains": chains}[which]
    index = {}
    rows = []
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
    # (the ext bodies' descriptors write their payloads to a scratch range behind the runs' output)
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
    out, st, nn, _ = call.run(g)
    b_out, b_st, b_nn = d_out.cpu().numpy(), status.cpu().numpy().view(np.uint16), nonces.cpu().numpy().view(np.uint64)
    for ri, r in enumerate(call.runs):
        nout = max(r.size - 33, 0)
        for j in range(len(r.bodies)):
            d, rec = index[("run", ri, j)], call.first[ri] + j
            assert st[rec] == b_st[d] and nn[rec] == b_nn[d], call.where(rec)
            if (st[rec] & 0xff) in (rx.ST_OK, rx.ST_CRYPTO):
                o = call.out_off[ri] + j * r.out_stride
                assert out[o:o + nout].tobytes() == b_out[o:o + nout].tobytes(), call.where(rec)
