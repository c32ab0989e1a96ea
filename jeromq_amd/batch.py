"""Device-resident batched seal/open over torch tensors (torch = HBM allocator + streams only).

All functions launch asynchronously on `stream` (default: torch's current
stream) and return immediately; the crypto runs in the gfx950 kernels of
libcurvezmq_mi355x.so.
"""
import ctypes

import numpy as np

from . import _lib


def _stream(stream):
    import torch
    if stream is None:
        return torch.cuda.current_stream().cuda_stream
    return getattr(stream, "cuda_stream", stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _need_cuda_u8(t, what):
    import torch
    if t is None or not t.is_cuda:
        raise ValueError(f"{what} must be a CUDA (HIP) tensor")
    if t.dtype != torch.uint8 and what not in ("desc",):
        raise ValueError(f"{what} must be uint8")


def subkeys(precom, direction, stream=None):
    """precom: (nkeys, 32) uint8 device tensor -> (nkeys, 32) subkeys for `direction`."""
    import torch
    _need_cuda_u8(precom, "precom")
    out = torch.empty_like(precom)
    _lib.check(_lib.lib().cz_subkeys(_ptr(out), _ptr(precom), precom.shape[0], direction, _stream(stream)),
               "cz_subkeys")
    return out


def seal_uniform(inp, in_stride, out, out_stride, count, length, subkey, counter0, flags8=None, stream=None):
    """Seal `count` payloads of `length` bytes (frame i at in[i*in_stride]) into MESSAGE
    bodies; body i goes to slot i = out[i*out_stride : (i+1)*out_stride].  With an out_stride
    that is a multiple of 128 below 2^25, or a multiple of 16 up to 256, the batch owns whole
    slots: slot bytes past the body are written as zeros; with any other stride they are left
    as they were (cz_seal_uniform in include/curvezmq_mi355x.h)."""
    _need_cuda_u8(inp, "in")
    _need_cuda_u8(out, "out")
    need_in = (count - 1) * in_stride + length if count else 0
    need_out = count * out_stride if count else 0
    if out_stride < length + _lib.CZ_MESSAGE_OVERHEAD and count > 1:
        raise ValueError("out_stride smaller than a MESSAGE body")
    if inp.numel() < need_in or out.numel() < need_out:
        raise ValueError("buffer too small for the batch")
    if flags8 is not None and flags8.numel() < count:
        raise ValueError("flags8 too small")
    _lib.check(_lib.lib().cz_seal_uniform(count, length, _ptr(inp), in_stride, _ptr(out), out_stride, _ptr(subkey),
                                          counter0, _ptr(flags8), _stream(stream)), "cz_seal_uniform")


FANOUT_SUB_DTYPE = np.dtype([("counter", "<u8"), ("key_idx", "<u4"), ("reserved", "<u4")])


def seal_fanout(payload, length, flags, subs, subkeys_t, out, out_stride, count, stream=None):
    """PUB fan-out: seal the ONE `length`-byte payload at payload[0] with MESSAGE flags byte `flags`
    for `count` subscribers; body i goes to out[i*out_stride] under subkey subs[i].key_idx and nonce
    subs[i].counter (subs: a device tensor of count 16-byte cz_fanout_sub records, FANOUT_SUB_DTYPE).
    The bytes are those of seal_batch with `count` descriptors sharing one in_off.  With an
    out_stride that is a multiple of 128 the batch owns whole slots (zeros past each body)."""
    _need_cuda_u8(payload, "payload")
    _need_cuda_u8(out, "out")
    _need_cuda_u8(subkeys_t, "subkeys")
    if subs is None or not subs.is_cuda:
        raise ValueError("subs must be a CUDA (HIP) tensor")
    if out_stride < length + _lib.CZ_MESSAGE_OVERHEAD:
        raise ValueError("out_stride smaller than a MESSAGE body")
    if count:
        if payload.numel() < length or out.numel() < (count - 1) * out_stride + length + _lib.CZ_MESSAGE_OVERHEAD:
            raise ValueError("buffer too small for the batch")
        if subs.numel() * subs.element_size() < count * FANOUT_SUB_DTYPE.itemsize:
            raise ValueError("subs too small")
    _lib.check(_lib.lib().cz_seal_fanout(count, length, _ptr(payload), flags, _ptr(subs), _ptr(subkeys_t), _ptr(out),
                                         out_stride, _stream(stream)), "cz_seal_fanout")


FANOUT_RUN_DTYPE = np.dtype([("payload_off", "<u8"), ("out_off", "<u8"), ("out_stride", "<u8"), ("len", "<u4"),
                             ("flags", "<u4"), ("first_sub", "<u4"), ("count", "<u4")])
FANOUT_WAVE_DTYPE = np.dtype([("run", "<u4"), ("first", "<u4")])


class FanoutPlan:
    """Host plan of a grouped fan-out (cz_plan_fanout): `waves` (FANOUT_WAVE_DTYPE) sorted by staging
    class, `class_count` = waves of the line / region / lane-wise class, `region_stride` = what sizes
    the region launch's LDS.  `to(device)` uploads the run and wave tables."""

    def __init__(self, runs_np, waves, class_count, region_stride):
        self.runs, self.waves = runs_np, waves
        self.class_count, self.region_stride = list(class_count), region_stride
        self.nruns, self.nwaves = len(runs_np), len(waves)
        self.d_runs = self.d_waves = None

    def to(self, device):
        import torch
        self.d_runs = torch.from_numpy(np.ascontiguousarray(self.runs).view(np.uint8).copy()).to(device)
        self.d_waves = torch.from_numpy(np.ascontiguousarray(self.waves).view(np.uint8).copy()).to(device)
        return self


def plan_fanout(runs_np, inp, out):
    """Plan the grouped fan-out of `runs_np` (FANOUT_RUN_DTYPE) reading `inp` and writing `out`: device
    tensors (or plain addresses), used for their 16-byte alignment only.  Returns a FanoutPlan."""
    r = np.ascontiguousarray(runs_np, dtype=FANOUT_RUN_DTYPE)
    a_in, a_out = (t if isinstance(t, int) else t.data_ptr() for t in (inp, out))
    nw, rs, cc = ctypes.c_uint32(), ctypes.c_uint32(), (ctypes.c_uint32 * 3)()
    L = _lib.lib()
    L.cz_plan_fanout(r.ctypes.data, len(r), a_in, a_out, None, 0, ctypes.byref(nw), cc, ctypes.byref(rs))
    waves = np.zeros(max(nw.value, 1), dtype=FANOUT_WAVE_DTYPE)
    _lib.check(L.cz_plan_fanout(r.ctypes.data, len(r), a_in, a_out, waves.ctypes.data, len(waves), ctypes.byref(nw),
                                cc, ctypes.byref(rs)), "cz_plan_fanout")
    return FanoutPlan(r, waves[:nw.value], cc, rs.value)


def _check_run_bounds(runs_np, inp, out, subs):
    """Every live run's payload, output range (whole slots where the run owns them) and subscriber
    records inside their tensors."""
    live = runs_np[runs_np["count"] > 0]
    if len(live):
        ln, cnt = live["len"].astype(np.uint64), live["count"].astype(np.uint64)
        nsubs = subs.numel() * subs.element_size() // FANOUT_SUB_DTYPE.itemsize
        st = live["out_stride"]
        owns = ((st % 128 == 0) & (st < (1 << 25))) | ((st % 16 == 0) & (st <= 256))   # whole slots are written
        last = np.where(owns, st, ln + np.uint64(33))
        if (np.any(live["payload_off"] + ln > np.uint64(inp.numel()))
                or np.any(live["out_off"] + (cnt - np.uint64(1)) * st + last > np.uint64(out.numel()))
                or np.any(live["first_sub"].astype(np.uint64) + cnt > np.uint64(nsubs))):
            raise ValueError("run out of bounds")


def seal_fanout_runs(plan, inp, subs, subkeys_t, out, stream=None):
    """Grouped PUB fan-out: every run of `plan` (plan_fanout(...).to(device)) sealed in one call of at
    most three launches; run r writes what seal_fanout writes for it alone.  The runs' output ranges
    must not overlap.  Bounds are checked against the plan's host copy of the runs."""
    _need_cuda_u8(inp, "in")
    _need_cuda_u8(out, "out")
    _need_cuda_u8(subkeys_t, "subkeys")
    if subs is None or not subs.is_cuda:
        raise ValueError("subs must be a CUDA (HIP) tensor")
    if plan.nruns and plan.d_runs is None:
        raise ValueError("plan not uploaded: plan.to(device)")
    _check_run_bounds(plan.runs, inp, out, subs)
    cc = (ctypes.c_uint32 * 3)(*plan.class_count)
    _lib.check(_lib.lib().cz_seal_fanout_runs(_ptr(plan.d_runs), plan.nruns, _ptr(plan.d_waves), cc,
                                              plan.region_stride, _ptr(inp), _ptr(subs), _ptr(subkeys_t), _ptr(out),
                                              _stream(stream)), "cz_seal_fanout_runs")


FANIN_SUB_DTYPE = np.dtype([("floor", "<u8"), ("key_idx", "<u4"), ("flags", "<u4")])
FANIN_RUN_DTYPE = np.dtype([("in_off", "<u8"), ("in_stride", "<u8"), ("out_off", "<u8"), ("out_stride", "<u8"),
                            ("size", "<u4"), ("first_sub", "<u4"), ("count", "<u4"), ("reserved", "<u4")])
FANIN_CHECK_NONCE, FANIN_FLOOR_IS_BODY = _lib.CZ_FANIN_CHECK_NONCE, _lib.CZ_FANIN_FLOOR_IS_BODY


class FaninPlan(FanoutPlan):
    """Host plan of a fan-in open (cz_plan_fanin): the runs (FANIN_RUN_DTYPE) and, as FanoutPlan, `waves`
    sorted by staging class, `class_count` and `region_stride`.  `to(device)` uploads the run and wave
    tables.  A caller may replace `waves` and `class_count` with a table of its own before `to`."""


def plan_fanin(runs_np, inp, out):
    """Plan the fan-in open of `runs_np` (FANIN_RUN_DTYPE) reading `inp` and writing `out`: device tensors
    (or plain addresses), used for their 16-byte alignment only.  Returns a FaninPlan."""
    r = np.ascontiguousarray(runs_np, dtype=FANIN_RUN_DTYPE)
    a_in, a_out = (t if isinstance(t, int) else t.data_ptr() for t in (inp, out))
    nw, rs, cc = ctypes.c_uint32(), ctypes.c_uint32(), (ctypes.c_uint32 * 3)()
    L = _lib.lib()
    L.cz_plan_fanin(r.ctypes.data, len(r), a_in, a_out, None, 0, ctypes.byref(nw), cc, ctypes.byref(rs))
    waves = np.zeros(max(nw.value, 1), dtype=FANOUT_WAVE_DTYPE)
    _lib.check(L.cz_plan_fanin(r.ctypes.data, len(r), a_in, a_out, waves.ctypes.data, len(waves), ctypes.byref(nw),
                               cc, ctypes.byref(rs)), "cz_plan_fanin")
    return FaninPlan(r, waves[:nw.value], cc, rs.value)


def _check_fanin_bounds(runs_np, inp, out, subs_np, nsubs, status, nonces):
    """Every live run's bodies, output range (whole slots where the run owns them) and record, status and
    nonce ranges inside their tensors; with the host copy of the records (`subs_np`), every
    FLOOR_IS_BODY offset's 16 bytes inside `inp`."""
    live = runs_np[runs_np["count"] > 0]
    if len(live):
        sz, cnt = live["size"].astype(np.uint64), live["count"].astype(np.uint64)
        nout = np.where(sz >= 33, sz - np.uint64(33), 0).astype(np.uint64)
        st = live["out_stride"]
        owns = ((st % 128 == 0) & (st < (1 << 25))) | ((st % 16 == 0) & (st <= 256))   # whole slots are written
        last = np.where(owns, st, nout)
        end = live["first_sub"].astype(np.uint64) + cnt
        if (np.any(live["in_off"] + (cnt - np.uint64(1)) * live["in_stride"] + sz > np.uint64(inp.numel()))
                or np.any(live["out_off"] + (cnt - np.uint64(1)) * st + last > np.uint64(out.numel()))
                or np.any(end > np.uint64(nsubs)) or np.any(end > np.uint64(status.numel()))
                or (nonces is not None and np.any(end > np.uint64(nonces.numel())))):
            raise ValueError("run out of bounds")
    if subs_np is not None and len(subs_np):
        body = (subs_np["flags"] & FANIN_FLOOR_IS_BODY) != 0
        if np.any(subs_np["floor"][body] > np.uint64(max(inp.numel(), 16) - 16)) or (body.any() and inp.numel() < 16):
            raise ValueError("FLOOR_IS_BODY offset out of bounds")


def open_fanin_runs(plan, inp, subs, subkeys_t, out, status, nonces=None, stream=None, subs_np=None):
    """Fan-in open: every run of `plan` (plan_fanin(...).to(device)) opened in one call of at most three
    launches, one lane per body.  subs: a device tensor of 16-byte cz_fanin_sub records (FANIN_SUB_DTYPE);
    body j of a run uses record, status (int16 / uint16 tensor) and nonce (int64 tensor, optional)
    first_sub + j.  Bounds are checked against the plan's host copy of the runs and, when given, the host
    copy of the records (`subs_np`: FLOOR_IS_BODY offsets)."""
    _need_cuda_u8(inp, "in")
    _need_cuda_u8(out, "out")
    _need_cuda_u8(subkeys_t, "subkeys")
    if subs is None or not subs.is_cuda or status is None or not status.is_cuda:
        raise ValueError("subs and status must be CUDA (HIP) tensors")
    if plan.nruns and plan.d_runs is None:
        raise ValueError("plan not uploaded: plan.to(device)")
    _check_fanin_bounds(plan.runs, inp, out, subs_np, subs.numel() * subs.element_size() // FANIN_SUB_DTYPE.itemsize,
                        status, nonces)
    cc = (ctypes.c_uint32 * 3)(*plan.class_count)
    _lib.check(_lib.lib().cz_open_fanin_runs(_ptr(plan.d_runs), plan.nruns, _ptr(plan.d_waves), cc, plan.region_stride,
                                             _ptr(inp), _ptr(subs), _ptr(subkeys_t), _ptr(out), _ptr(status),
                                             _ptr(nonces), _stream(stream)), "cz_open_fanin_runs")


FANOUT_TILE_DTYPE = np.dtype([("run", "<u4"), ("first", "<u4"), ("first_block", "<u4"), ("nblocks", "<u4"),
                              ("part", "<u4"), ("nseg", "<u4")])
FANOUT_JOIN_DTYPE = np.dtype([("run", "<u4"), ("first", "<u4"), ("part", "<u4"), ("nseg", "<u4")])


class FanoutSplitPlan:
    """Host plan of a split fan-out (cz_plan_fanout_split): `tiles` (FANOUT_TILE_DTYPE), one per wave of
    64 subscribers and per segment, sorted by class; `class_count` = tiles of the line / lane-wise class;
    `joins` (FANOUT_JOIN_DTYPE), one per wave of a split run; `npart` = 64-byte partial records the work
    buffer must hold.  `to(device)` uploads the three tables.  A caller may replace `tiles`, `joins`,
    `class_count` and `npart` with tables of its own before `to`."""

    def __init__(self, runs_np, tiles, class_count, joins, npart):
        self.runs, self.tiles, self.joins = runs_np, tiles, joins
        self.class_count, self.npart = list(class_count), npart
        self.nruns = len(runs_np)
        self.d_runs = self.d_tiles = self.d_joins = None

    def to(self, device):
        import torch

        def up(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dt).view(np.uint8).copy()).to(device)
        self.d_runs = up(self.runs, FANOUT_RUN_DTYPE)
        self.d_tiles = up(self.tiles, FANOUT_TILE_DTYPE)
        self.d_joins = up(self.joins, FANOUT_JOIN_DTYPE)
        return self


def plan_fanout_split(runs_np, inp, out, seg_blocks=0):
    """Plan the split fan-out of `runs_np` (FANOUT_RUN_DTYPE) reading `inp` (a device tensor or a plain
    address, used for its 16-byte alignment only) and writing `out` (not looked at: the kernel picks the
    emitter from the output's alignment itself).  seg_blocks 0: the engine's choice for a batch of this
    size.  Returns a FanoutSplitPlan."""
    r = np.ascontiguousarray(runs_np, dtype=FANOUT_RUN_DTYPE)
    a_in = inp if isinstance(inp, int) else inp.data_ptr()
    nt, nj, npart, cc = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), (ctypes.c_uint32 * 2)()
    L = _lib.lib()
    L.cz_plan_fanout_split(r.ctypes.data, len(r), a_in, seg_blocks, None, 0, ctypes.byref(nt), cc, None, 0,
                           ctypes.byref(nj), ctypes.byref(npart))
    tiles = np.zeros(max(nt.value, 1), dtype=FANOUT_TILE_DTYPE)
    joins = np.zeros(max(nj.value, 1), dtype=FANOUT_JOIN_DTYPE)
    _lib.check(L.cz_plan_fanout_split(r.ctypes.data, len(r), a_in, seg_blocks, tiles.ctypes.data, len(tiles),
                                      ctypes.byref(nt), cc, joins.ctypes.data, len(joins), ctypes.byref(nj),
                                      ctypes.byref(npart)), "cz_plan_fanout_split")
    return FanoutSplitPlan(r, tiles[:nt.value], cc, joins[:nj.value], npart.value)


def seal_fanout_split(plan, inp, subs, subkeys_t, out, work=None, stream=None):
    """Split PUB fan-out: every run of `plan` (plan_fanout_split(...).to(device)) sealed on a subscriber x
    segment grid in at most three launches; run r writes what seal_fanout writes for it alone.  The runs'
    output ranges must not overlap.  `work`: 64 * plan.npart bytes of device scratch, allocated when not
    given.  Bounds are checked against the plan's host copy of the runs."""
    import torch
    _need_cuda_u8(inp, "in")
    _need_cuda_u8(out, "out")
    _need_cuda_u8(subkeys_t, "subkeys")
    if subs is None or not subs.is_cuda:
        raise ValueError("subs must be a CUDA (HIP) tensor")
    if plan.nruns and plan.d_runs is None:
        raise ValueError("plan not uploaded: plan.to(device)")
    _check_run_bounds(plan.runs, inp, out, subs)
    if work is None:
        work = torch.empty(max(plan.npart, 1) * 64, dtype=torch.uint8, device=out.device)
    elif work.numel() * work.element_size() < 64 * plan.npart:
        raise ValueError("work smaller than 64 * plan.npart bytes")
    cc = (ctypes.c_uint32 * 2)(*plan.class_count)
    _lib.check(_lib.lib().cz_seal_fanout_split(_ptr(plan.d_runs), plan.nruns, _ptr(plan.d_tiles), cc,
                                               _ptr(plan.d_joins), len(plan.joins), _ptr(inp), _ptr(subs),
                                               _ptr(subkeys_t), _ptr(out), _ptr(work), _stream(stream)),
               "cz_seal_fanout_split")
    return work


class FaninSplitPlan(FanoutSplitPlan):
    """Host plan of a split fan-in open (cz_plan_fanin_split): the runs (FANIN_RUN_DTYPE) and, as
    FanoutSplitPlan, `tiles` (one per wave of 64 bodies and per segment, sorted by class), `class_count`,
    `joins` and `npart`.  `to(device)` uploads the three tables.  A caller may replace `tiles`, `joins`,
    `class_count` and `npart` with tables of its own before `to`."""

    def to(self, device):
        import torch

        def up(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dt).view(np.uint8).copy()).to(device)
        self.d_runs = up(self.runs, FANIN_RUN_DTYPE)
        self.d_tiles = up(self.tiles, FANOUT_TILE_DTYPE)
        self.d_joins = up(self.joins, FANOUT_JOIN_DTYPE)
        return self


def plan_fanin_split(runs_np, inp, out, seg_blocks=0):
    """Plan the split fan-in open of `runs_np` (FANIN_RUN_DTYPE) reading `inp` and writing `out`: device
    tensors (or plain addresses), used as addresses only (`inp` for the tiles' class).  seg_blocks 0: the
    length flush_in picks for a flush of the runs' total body bytes.  Returns a FaninSplitPlan."""
    r = np.ascontiguousarray(runs_np, dtype=FANIN_RUN_DTYPE)
    a_in, a_out = (t if isinstance(t, int) else t.data_ptr() for t in (inp, out))
    nt, nj, npart, cc = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), (ctypes.c_uint32 * 2)()
    L = _lib.lib()
    L.cz_plan_fanin_split(r.ctypes.data, len(r), a_in, a_out, seg_blocks, None, 0, ctypes.byref(nt), cc, None, 0,
                          ctypes.byref(nj), ctypes.byref(npart))
    tiles = np.zeros(max(nt.value, 1), dtype=FANOUT_TILE_DTYPE)
    joins = np.zeros(max(nj.value, 1), dtype=FANOUT_JOIN_DTYPE)
    _lib.check(L.cz_plan_fanin_split(r.ctypes.data, len(r), a_in, a_out, seg_blocks, tiles.ctypes.data, len(tiles),
                                     ctypes.byref(nt), cc, joins.ctypes.data, len(joins), ctypes.byref(nj),
                                     ctypes.byref(npart)), "cz_plan_fanin_split")
    return FaninSplitPlan(r, tiles[:nt.value], cc, joins[:nj.value], npart.value)


def open_fanin_split(plan, inp, subs, subkeys_t, out, status, nonces=None, work=None, stream=None, subs_np=None):
    """Split fan-in open: every run of `plan` (plan_fanin_split(...).to(device)) opened on a connection x
    segment grid in at most three launches; every run gets what open_fanin_runs writes for it.  Records,
    statuses and nonces as open_fanin_runs.  `work`: 64 * plan.npart bytes of device scratch, allocated
    when not given.  Bounds are checked as open_fanin_runs checks them."""
    import torch
    _need_cuda_u8(inp, "in")
    _need_cuda_u8(out, "out")
    _need_cuda_u8(subkeys_t, "subkeys")
    if subs is None or not subs.is_cuda or status is None or not status.is_cuda:
        raise ValueError("subs and status must be CUDA (HIP) tensors")
    if plan.nruns and plan.d_runs is None:
        raise ValueError("plan not uploaded: plan.to(device)")
    _check_fanin_bounds(plan.runs, inp, out, subs_np, subs.numel() * subs.element_size() // FANIN_SUB_DTYPE.itemsize,
                        status, nonces)
    if work is None:
        work = torch.empty(max(plan.npart, 1) * 64, dtype=torch.uint8, device=out.device)
    elif work.numel() * work.element_size() < 64 * plan.npart:
        raise ValueError("work smaller than 64 * plan.npart bytes")
    cc = (ctypes.c_uint32 * 2)(*plan.class_count)
    _lib.check(_lib.lib().cz_open_fanin_split(_ptr(plan.d_runs), plan.nruns, _ptr(plan.d_tiles), cc,
                                              _ptr(plan.d_joins), len(plan.joins), _ptr(inp), _ptr(subs),
                                              _ptr(subkeys_t), _ptr(out), _ptr(work), _ptr(status), _ptr(nonces),
                                              _stream(stream)), "cz_open_fanin_split")
    return work


def seal_uniform_box(box, box_stride, out, out_stride, count, length, subkey, counter0, stream=None):
    """Uniform seal from the reference's box layout: slot i of `box` holds 0^32 || flags ||
    payload (length = payload bytes), as CurveClientMechanism.encode hands it to Curve.afternm."""
    _need_cuda_u8(box, "box")
    _need_cuda_u8(out, "out")
    if count:  # (like seal_uniform, the batch owns whole output slots)
        if box.numel() < (count - 1) * box_stride + length + 33 or out.numel() < count * out_stride:
            raise ValueError("seal_uniform_box: buffers smaller than the batch")
    _lib.check(_lib.lib().cz_seal_uniform_box(count, length, _ptr(box), box_stride, _ptr(out), out_stride,
                                              _ptr(subkey), counter0, _stream(stream)), "cz_seal_uniform_box")


def open_uniform(inp, in_stride, out, out_stride, count, size, subkey, floor0, status, check=True, stream=None):
    """Open `count` bodies of `size` bytes of one connection, in order; payload i goes to
    slot out[i*out_stride : (i+1)*out_stride] (whole slots owned by the batch)."""
    _need_cuda_u8(inp, "in")
    _need_cuda_u8(out, "out")
    if count and (inp.numel() < (count - 1) * in_stride + size or status.numel() < count):
        raise ValueError("buffer too small for the batch")
    if count and size >= 33 and out.numel() < count * out_stride:
        raise ValueError("output too small for the batch (needs count * out_stride bytes)")
    _lib.check(_lib.lib().cz_open_uniform(count, size, _ptr(inp), in_stride, _ptr(out), out_stride, _ptr(subkey),
                                          floor0, 1 if check else 0, _ptr(status), _stream(stream)),
               "cz_open_uniform")


def _check_desc_bounds(desc_np, in_bytes, out_bytes, nkeys, seal):
    ln = desc_np["len"].astype(np.uint64)
    olen = ln + np.uint64(33) if seal else np.where(ln >= 33, ln - np.uint64(33), 0).astype(np.uint64)
    if len(desc_np) and (np.any(desc_np["in_off"] + ln > np.uint64(in_bytes))
                         or np.any(desc_np["out_off"] + olen > np.uint64(out_bytes))
                         or np.any(desc_np["key_idx"] >= nkeys)):
        raise ValueError("descriptor out of bounds")


def seal_batch(desc, count, inp, out, subkeys_t, order=None, stream=None, desc_np=None):
    """desc: device tensor holding `count` cz_frame_desc (40 B each).  If desc_np (the host
    copy, numpy DESC dtype) is given, bounds are checked before the launch."""
    _need_cuda_u8(inp, "in")
    _need_cuda_u8(out, "out")
    if desc_np is not None:
        _check_desc_bounds(desc_np, inp.numel(), out.numel(), subkeys_t.shape[0], True)
    _lib.check(_lib.lib().cz_seal_batch(_ptr(desc), _ptr(order), count, _ptr(inp), _ptr(out), _ptr(subkeys_t),
                                        _stream(stream)), "cz_seal_batch")


def open_batch(desc, count, inp, out, subkeys_t, status, nonces=None, order=None, stream=None, desc_np=None):
    _need_cuda_u8(inp, "in")
    _need_cuda_u8(out, "out")
    if desc_np is not None:
        _check_desc_bounds(desc_np, inp.numel(), out.numel(), subkeys_t.shape[0], False)
    _lib.check(_lib.lib().cz_open_batch(_ptr(desc), _ptr(order), count, _ptr(inp), _ptr(out), _ptr(subkeys_t),
                                        _ptr(status), _ptr(nonces), _stream(stream)), "cz_open_batch")


def _check_relay_bounds(desc_np, to_np, count, in_bytes, out_bytes, nkeys, nstatus, nnonces):
    """Every frame's body inside `in`, its re-sealed body of the same size inside `out`, both key indices
    inside the table, and one status (and nonce) entry per frame."""
    if nstatus < count or (nnonces is not None and nnonces < count):
        raise ValueError("status / nonces hold fewer than count records")
    if desc_np is not None:
        if len(desc_np) < count:
            raise ValueError("desc_np holds fewer than count descriptors")
        d = desc_np[:count]
        ln = d["len"].astype(np.uint64)
        if count and (np.any(d["in_off"] + ln > np.uint64(in_bytes)) or np.any(d["out_off"] + ln > np.uint64(out_bytes))
                      or np.any(d["key_idx"] >= nkeys) or np.any(d["prev"] >= count)):
            raise ValueError("descriptor out of bounds")
    if to_np is not None:
        if len(to_np) < count:
            raise ValueError("to_np holds fewer than count records")
        if count and np.any(to_np["key_idx"][:count] >= nkeys):
            raise ValueError("outbound key index out of bounds")


def relay_batch(desc, to, count, inp, out, subkeys_t, status, nonces=None, order=None, stream=None, desc_np=None,
                to_np=None):
    """Relay `count` received MESSAGE bodies (cz_relay_batch): frame i, read as open_batch reads desc[i],
    is re-sealed at out[desc[i].out_off] with the same size under subkey to[i].key_idx and nonce
    to[i].counter (to: a device tensor of 16-byte cz_fanout_sub records, FANOUT_SUB_DTYPE).  status and
    nonces as open_batch; a rejected frame's output bytes are zeros.  The plaintext never reaches memory.
    With the host copies desc_np / to_np, bounds and both key indices are checked before the launch."""
    _need_cuda_u8(inp, "in")
    _need_cuda_u8(out, "out")
    _need_cuda_u8(subkeys_t, "subkeys")
    if desc is None or not desc.is_cuda or to is None or not to.is_cuda or status is None or not status.is_cuda:
        raise ValueError("desc, to and status must be CUDA (HIP) tensors")
    if (desc.numel() * desc.element_size() < count * DESC_DTYPE.itemsize
            or to.numel() * to.element_size() < count * FANOUT_SUB_DTYPE.itemsize
            or (order is not None and order.numel() < count)):
        raise ValueError("desc / to / order hold fewer than count records")
    _check_relay_bounds(desc_np, to_np, count, inp.numel(), out.numel(), subkeys_t.shape[0], status.numel(),
                        None if nonces is None else nonces.numel())
    _lib.check(_lib.lib().cz_relay_batch(_ptr(desc), _ptr(to), _ptr(order), count, _ptr(inp), _ptr(out),
                                         _ptr(subkeys_t), _ptr(status), _ptr(nonces), _stream(stream)),
               "cz_relay_batch")


def _check_relay_uniform_bounds(in_bytes, in_stride, out_bytes, out_stride, count, size, nstatus):
    """`count` bodies inside `in`, their output range (whole slots where the batch owns them) inside
    `out`, one status entry per frame."""
    if not count:
        return
    if count > 1 and (in_stride < size or out_stride < size):
        raise ValueError("stride smaller than a body")
    owns = (out_stride % 128 == 0 and out_stride < (1 << 25)) or (out_stride % 16 == 0 and out_stride <= 256)
    last = out_stride if owns and out_stride > size else size
    if in_bytes < (count - 1) * in_stride + size or out_bytes < (count - 1) * out_stride + last or nstatus < count:
        raise ValueError("buffer too small for the batch")


def relay_uniform(inp, in_stride, out, out_stride, count, size, subkey_in, floor0, subkey_out, counter0, status,
                  check=True, stream=None):
    """Relay `count` bodies of `size` bytes of one connection, in order (the chain rule of open_uniform), to
    one connection: body i is re-sealed at out[i*out_stride] under subkey_out with nonce counter0 + i
    (cz_relay_uniform).  A rejected frame's bytes are zeros and its counter is skipped.  Output
    ownership by out_stride as seal_uniform.  Input and output must not overlap."""
    _need_cuda_u8(inp, "in")
    _need_cuda_u8(out, "out")
    _need_cuda_u8(subkey_in, "subkey_in")
    _need_cuda_u8(subkey_out, "subkey_out")
    if status is None or not status.is_cuda:
        raise ValueError("status must be a CUDA (HIP) tensor")
    if subkey_in.numel() < 32 or subkey_out.numel() < 32:
        raise ValueError("a subkey is 32 bytes")
    _check_relay_uniform_bounds(inp.numel(), in_stride, out.numel(), out_stride, count, size, status.numel())
    _lib.check(_lib.lib().cz_relay_uniform(count, size, _ptr(inp), in_stride, _ptr(out), out_stride, _ptr(subkey_in),
                                           floor0, 1 if check else 0, _ptr(subkey_out), counter0, _ptr(status),
                                           _stream(stream)), "cz_relay_uniform")


def open_streams(streams, wire, results, desc, out, subkeys_t, status, nonces=None, maxmsgsize=-1, slot_align=128,
                 desc_cap=None, out_cap=None, stream=None):
    """Parse and open many received streams where they lie (cz_open_streams): `streams` a device tensor of
    wire.V2_STREAM_DTYPE records, `wire` the received bytes (readable for 16 bytes past the last stream),
    `results` / `desc` / `status` / `nonces` device tensors for one record per stream / frame, `out` the
    plaintext slots.  Scan, one synchronisation for the totals, emit, open.  Returns (rc, nframes,
    slot_bytes): rc is CZ_OK, or CZ_ENOMEM with the totals filled and nothing opened when they exceed
    desc_cap / out_cap (default: what `desc` / `out` hold).  Any other failure raises."""
    from .wire import V2_STREAM_DTYPE
    _need_cuda_u8(wire, "wire")
    _need_cuda_u8(out, "out")
    count = streams.numel() // V2_STREAM_DTYPE.itemsize
    if desc_cap is None:
        desc_cap = desc.numel() * desc.element_size() // DESC_DTYPE.itemsize
    if out_cap is None:
        out_cap = out.numel()
    if status.numel() * status.element_size() < 2 * desc_cap or (
            nonces is not None and nonces.numel() * nonces.element_size() < 8 * desc_cap):
        raise ValueError("status / nonces hold fewer than desc_cap records")
    tot = _lib.cz_v2_totals()
    rc = _lib.lib().cz_open_streams(_ptr(streams), count, _ptr(wire), maxmsgsize, slot_align, _ptr(results), _ptr(desc),
                                    desc_cap, _ptr(out), out_cap, _ptr(subkeys_t), _ptr(status), _ptr(nonces),
                                    ctypes.byref(tot), _stream(stream))
    if rc != _lib.CZ_ENOMEM:
        _lib.check(rc, "cz_open_streams")
    return rc, int(tot.nframes), int(tot.slot_bytes)


RELAY_STREAM_RESULT_DTYPE = np.dtype([("ok_bytes", "<u8"), ("whole_bytes", "<u8"), ("peer_nonce", "<u8"),
                                      ("ok_frames", "<u4"), ("fail_status", "<u2"), ("reserved", "<u2")])
assert RELAY_STREAM_RESULT_DTYPE.itemsize == 32


def _nbytes(t):
    return t.numel() * t.element_size()


def _check_relay_streams_bounds(count, nto, nscan, nresults, desc_cap, ndesc, nto_frames, nstatus, nnonces, wire_bytes,
                                out_bytes, streams_np=None, to_np=None, nkeys=None):
    """One outbound record, scan result and cut result per stream; desc_cap descriptors, outbound records,
    statuses and nonces per frame; `out` as long as `wire`; with the host copies, every stream and the 16
    readable bytes behind it inside `wire`, and both key indices inside the table."""
    if nto < count or nscan < count or nresults < count:
        raise ValueError("to / scan / results hold fewer than one record per stream")
    if ndesc < desc_cap or nto_frames < desc_cap or nstatus < desc_cap or nnonces < desc_cap:
        raise ValueError("desc / to_frames / status / nonces hold fewer than desc_cap records")
    if out_bytes < wire_bytes:
        raise ValueError("out is shorter than wire: it takes the same offsets")
    if streams_np is not None and count:
        s = streams_np[:count]
        if len(s) < count or np.any(s["off"] + s["len"] + np.uint64(16) > np.uint64(wire_bytes)):
            raise ValueError("stream out of bounds (wire must be readable for 16 bytes past its last stream)")
        if nkeys is not None and np.any(s["key_idx"] >= nkeys):
            raise ValueError("inbound key index out of bounds")
    if to_np is not None and count:
        if len(to_np) < count or (nkeys is not None and np.any(to_np["key_idx"][:count] >= nkeys)):
            raise ValueError("outbound key index out of bounds")


def relay_streams(streams, to, wire, out, scan, desc, to_frames, subkeys_t, status, nonces, results, maxmsgsize=-1,
                  stream=None, desc_cap=None, streams_np=None, to_np=None):
    """Re-seal many received V2 streams wire to wire (cz_relay_streams): `streams` a device tensor of
    wire.V2_STREAM_DTYPE records, `to` one FANOUT_SUB_DTYPE record per stream (the outbound counter of its first
    frame and the outbound subkey), `wire` the received bytes (readable for 16 bytes past the last stream), `out`
    the same tensor (in place) or one of at least its size that takes the same offsets.  `scan` / `results` hold
    one V2_STREAM_RESULT_DTYPE / RELAY_STREAM_RESULT_DTYPE record per stream; `desc` / `to_frames` / `status` /
    `nonces` one record per frame.  Scan, one synchronisation for the totals, emit, relay, cut.  Of every
    stream, send results[s].ok_bytes (or whole_bytes) and nothing behind them.  Returns (rc, nframes): rc is
    CZ_OK, or CZ_ENOMEM with nframes filled and nothing written when it exceeds desc_cap (default: what `desc`
    holds).  Any other failure raises.  With the host copies streams_np / to_np, bounds and key indices are
    checked before the launch."""
    from .wire import V2_STREAM_DTYPE, V2_STREAM_RESULT_DTYPE
    _need_cuda_u8(wire, "wire")
    _need_cuda_u8(out, "out")
    _need_cuda_u8(subkeys_t, "subkeys")
    for name, t in (("streams", streams), ("to", to), ("scan", scan), ("desc", desc), ("to_frames", to_frames),
                    ("status", status), ("nonces", nonces), ("results", results)):
        if t is None or not t.is_cuda:
            raise ValueError(f"{name} must be a CUDA (HIP) tensor")
    count = _nbytes(streams) // V2_STREAM_DTYPE.itemsize
    if desc_cap is None:
        desc_cap = _nbytes(desc) // DESC_DTYPE.itemsize
    _check_relay_streams_bounds(count, _nbytes(to) // FANOUT_SUB_DTYPE.itemsize,
                                _nbytes(scan) // V2_STREAM_RESULT_DTYPE.itemsize,
                                _nbytes(results) // RELAY_STREAM_RESULT_DTYPE.itemsize, desc_cap,
                                _nbytes(desc) // DESC_DTYPE.itemsize, _nbytes(to_frames) // FANOUT_SUB_DTYPE.itemsize,
                                _nbytes(status) // 2, _nbytes(nonces) // 8, wire.numel(), out.numel(), streams_np, to_np,
                                subkeys_t.shape[0])
    tot = _lib.cz_v2_totals()
    rc = _lib.lib().cz_relay_streams(_ptr(streams), _ptr(to), count, _ptr(wire), _ptr(out), maxmsgsize, _ptr(scan),
                                     _ptr(desc), _ptr(to_frames), desc_cap, _ptr(subkeys_t), _ptr(status), _ptr(nonces),
                                     _ptr(results), ctypes.byref(tot), _stream(stream))
    if rc != _lib.CZ_ENOMEM:
        _lib.check(rc, "cz_relay_streams")
    return rc, int(tot.nframes)


def fill(buf, seed, stream=None):
    """Counter-based SplitMix64 synthetic bytes (tests/cz_testlib.py splitmix_words)."""
    _lib.check(_lib.lib().cz_fill(_ptr(buf), buf.numel() * buf.element_size(), seed, _stream(stream)), "cz_fill")


def plan_order(desc_np):
    """Frame indices sorted by decreasing length (balances lanes of a ragged batch)."""
    count = len(desc_np)
    order = np.zeros(count, dtype=np.uint32)
    d = np.ascontiguousarray(desc_np)
    _lib.check(_lib.lib().cz_plan_order(d.ctypes.data, count, order.ctypes.data), "cz_plan_order")
    return order


DESC_DTYPE = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("len", "<u4"), ("key_idx", "<u4"),
                       ("counter", "<u8"), ("flags", "<u4"), ("prev", "<i4")])

SEGMENT_DTYPE = np.dtype([("frame", "<u4"), ("first_block", "<u4"), ("nblocks", "<u4"), ("part", "<u4")])
COMBINE_DTYPE = np.dtype([("frame", "<u4"), ("part0", "<u4"), ("nseg", "<u4"), ("reserved", "<u4")])
SEG_BLOCKS = 128  # 8 KiB of box per lane (Zipf sweep: 64 -> 1664, 128 -> 1687-1709, 160 -> 1707, 192 -> 1671 GiB/s)


class SegmentPlan:
    """Host plan for a ragged batch: frames longer than 1.5 x seg_blocks are split
    into seg_blocks-block segments (cz_plan_segments).  `to(device)` uploads the
    segment and combine lists and allocates the partial-record workspace (records=2: the two
    planes of 64-byte records per part that relay_segments needs)."""

    def __init__(self, desc_np, open_=False, seg_blocks=SEG_BLOCKS):
        d = np.ascontiguousarray(desc_np)
        count = len(d)
        nseg, ncomb, npart = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        L = _lib.lib()
        L.cz_plan_segments(d.ctypes.data, count, int(open_), seg_blocks, None, 0, ctypes.byref(nseg), None, 0,
                           ctypes.byref(ncomb), ctypes.byref(npart))
        self.segments = np.zeros(max(nseg.value, 1), dtype=SEGMENT_DTYPE)
        self.combines = np.zeros(max(ncomb.value, 1), dtype=COMBINE_DTYPE)
        _lib.check(L.cz_plan_segments(d.ctypes.data, count, int(open_), seg_blocks, self.segments.ctypes.data,
                                      len(self.segments), ctypes.byref(nseg), self.combines.ctypes.data,
                                      len(self.combines), ctypes.byref(ncomb), ctypes.byref(npart)),
                   "cz_plan_segments")
        self.nseg, self.ncomb, self.npart = nseg.value, ncomb.value, npart.value
        self.segments = self.segments[:self.nseg]
        self.combines = self.combines[:self.ncomb]
        self.d_seg = self.d_comb = self.d_work = None

    def to(self, device, records=1):
        import torch
        if records not in (1, 2):
            raise ValueError("records: 1 (seal / open) or 2 (relay)")
        self.d_seg = torch.from_numpy(self.segments.view(np.uint8).copy()).to(device)
        self.d_comb = torch.from_numpy(self.combines.view(np.uint8).copy()).to(device)
        self.d_work = torch.empty(max(self.npart, 1) * 64 * records, dtype=torch.uint8, device=device)
        return self


def seal_segments(desc, plan, inp, out, subkeys_t, stream=None, desc_np=None):
    """Ragged seal with long frames split across lanes (same output as seal_batch)."""
    _need_cuda_u8(inp, "in")
    _need_cuda_u8(out, "out")
    if desc_np is not None:
        _check_desc_bounds(desc_np, inp.numel(), out.numel(), subkeys_t.shape[0], True)
    _lib.check(_lib.lib().cz_seal_segments(_ptr(desc), _ptr(plan.d_seg), plan.nseg, _ptr(plan.d_comb), plan.ncomb,
                                           _ptr(inp), _ptr(out), _ptr(subkeys_t), _ptr(plan.d_work),
                                           _stream(stream)), "cz_seal_segments")


def open_segments(desc, plan, inp, out, subkeys_t, status, nonces=None, stream=None, desc_np=None):
    """Ragged open with long frames split across lanes (same output as open_batch)."""
    _need_cuda_u8(inp, "in")
    _need_cuda_u8(out, "out")
    if desc_np is not None:
        _check_desc_bounds(desc_np, inp.numel(), out.numel(), subkeys_t.shape[0], False)
    _lib.check(_lib.lib().cz_open_segments(_ptr(desc), _ptr(plan.d_seg), plan.nseg, _ptr(plan.d_comb), plan.ncomb,
                                           _ptr(inp), _ptr(out), _ptr(subkeys_t), _ptr(plan.d_work), _ptr(status),
                                           _ptr(nonces), _stream(stream)), "cz_open_segments")


def relay_segments(desc, to, plan, inp, out, subkeys_t, status, nonces=None, stream=None, desc_np=None, to_np=None):
    """Ragged relay with long bodies split across lanes (cz_relay_segments; same output, status and nonces
    as relay_batch).  plan: SegmentPlan(desc_np, open_=True, ...).to(device, records=2) -- the plan an
    open_segments of the same descriptors takes, with 128 bytes of workspace per part.  Input and output
    must not overlap.  With the host copies desc_np / to_np, bounds and both key indices are checked
    before the launch."""
    _need_cuda_u8(inp, "in")
    _need_cuda_u8(out, "out")
    _need_cuda_u8(subkeys_t, "subkeys")
    if desc is None or not desc.is_cuda or to is None or not to.is_cuda or status is None or not status.is_cuda:
        raise ValueError("desc, to and status must be CUDA (HIP) tensors")
    count = desc.numel() * desc.element_size() // DESC_DTYPE.itemsize
    if to.numel() * to.element_size() < count * FANOUT_SUB_DTYPE.itemsize:
        raise ValueError("to holds fewer records than desc")
    if plan.d_seg is None or plan.d_work is None or plan.d_work.numel() < 128 * plan.npart:
        raise ValueError("plan.d_work holds fewer than 128 bytes per part: SegmentPlan.to(device, records=2)")
    if plan.nseg and (int(plan.segments["frame"].max()) >= count):
        raise ValueError("plan names a frame past desc")
    _check_relay_bounds(desc_np, to_np, count, inp.numel(), out.numel(), subkeys_t.shape[0], status.numel(),
                        None if nonces is None else nonces.numel())
    _lib.check(_lib.lib().cz_relay_segments(_ptr(desc), _ptr(to), _ptr(plan.d_seg), plan.nseg, _ptr(plan.d_comb),
                                            plan.ncomb, plan.npart, _ptr(inp), _ptr(out), _ptr(subkeys_t),
                                            _ptr(plan.d_work), _ptr(status), _ptr(nonces), _stream(stream)),
               "cz_relay_segments")
