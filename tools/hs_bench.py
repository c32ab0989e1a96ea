#!/usr/bin/env python3
"""Latency of the batched CURVE handshake (cz_acceptor, or cz_connector with --side client) against the
per-connection one (cz_hs).

For N in {1, 64, 1024, 16384, 131072}: wall clock around the synchronous cz_acceptor_hello (stage 1)
and cz_acceptor_initiate (stage 2) calls, after one warm-up round, median of --reps rounds.  The
commands are generated once, outside the timed region, by the CPU model of tests/hs_model.py; the
C entry points are called directly, so no Python packing is timed.  Baseline in the same run: 64
cz_hs server objects driven one after another from construction through HELLO -> READY.

Command generation: connection i uses client i % POOL and the injected server short-term secret
i % POOL, with injected entropy, so the CPU side needs POOL key agreements, not N, and a round's
WELCOMEs (hence the INITIATEs made from them) are the same every round.  The device work per lane
does not depend on that.  `stage1_getrandom_ms` is stage 1 drawing its secrets and entropy from
getrandom, as in production.

--side client times the three cz_connector stages (hello, welcome, ready) the same way: the server's
WELCOMEs and READYs come from the CPU model, outside the timed region, for the injected short-term
secrets and vouch nonces of POOL connections of one client; the baseline is 64 cz_hs clients one after
another, constructor through READY.  `hello_getrandom_ms` is stage 1 drawing its secrets from getrandom.

--handover times what follows the handshake instead: N accepted sessions into the batching engine and out
of the acceptor's slot table, per slot (cz_engine_add_accepted + cz_acceptor_release in a loop) against
the bulk calls (cz_engine_add_accepted_batch + cz_acceptor_release_batch), the same for
cz_engine_remove_conn against cz_engine_remove_conns, and the two handshake stages beside them
(handover_main).

Writes one JSON (default profiles/hs_batch/hs_batch.json, hs_connect.json for the client, hs_handover.json
for --handover) and prints it."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SERVER_PUB = bytes.fromhex("54FCBA24E93249969316FB617C872BB0C1D1FF14800427C594CBFACF1BC2D652")
SERVER_SEC = bytes.fromhex("8E0BDD697628B91D8F245587EE95C5B04D48963F79259877B49CD9063AEAD3B7")
POOL = 64
SIZES = (1, 64, 1024, 16384, 131072)


def make_pool():
    import hs_model as M
    from cz_testlib import splitmix_bytes
    pool = []
    for i in range(POOL):
        b = splitmix_bytes(176, 990000 + i)
        c = {"csec": b[0:32], "ceph": b[32:64], "seph": b[64:96], "entropy": b[96:160], "vnonce": b[160:176]}
        c["cpub"] = M.public_key(c["csec"])
        c["hello"] = M.client_hello(SERVER_PUB, c["ceph"])
        c["welcome"], _ = M.server_welcome(c["hello"], SERVER_SEC, c["seph"], c["entropy"])
        c["initiate"] = M.client_initiate(c["welcome"], c["cpub"], c["csec"], SERVER_PUB, c["ceph"], c["vnonce"])
        pool.append(c)
    return pool


class Batch:
    """prebuilt arguments of the two stage calls for n connections"""

    def __init__(self, pool, n):
        from jeromq_amd import _lib
        self.n = n
        idx = np.arange(n) % POOL
        self.hello = np.frombuffer(b"".join(c["hello"] for c in pool), dtype=np.uint8).reshape(POOL, 200)[idx].copy()
        ini = [c["initiate"] for c in pool]
        self.isize = len(ini[0])
        assert all(len(x) == self.isize for x in ini)
        self.init = np.frombuffer(b"".join(ini), dtype=np.uint8).reshape(POOL, self.isize)[idx].copy()
        self.secrets = np.frombuffer(b"".join(c["seph"] for c in pool), dtype=np.uint8).reshape(POOL, 32)[idx].copy()
        self.entropy = np.frombuffer(b"".join(c["entropy"] for c in pool), dtype=np.uint8).reshape(POOL, 64)[idx].copy()
        self.hoff = (np.arange(n, dtype=np.uint64) * np.uint64(200))
        self.hsize = np.full(n, 200, dtype=np.uint32)
        self.ioff = (np.arange(n, dtype=np.uint64) * np.uint64(self.isize))
        self.isz = np.full(n, self.isize, dtype=np.uint32)
        self.res = (_lib.cz_accept_result * n)()
        self.reply = np.zeros(n * 288, dtype=np.uint8)
        self.slots = np.zeros(n, dtype=np.int32)
        self.welcome0, self.ready0 = pool[0]["welcome"], None

    def stage1(self, L, acc, injected=True):
        t0 = time.perf_counter()
        rc = L.cz_acceptor_hello(acc, self.n, self.hello.ctypes.data, self.hello.nbytes, self.hoff.ctypes.data,
                                 self.hsize.ctypes.data, self.reply.ctypes.data, 168, self.res,
                                 self.secrets.ctypes.data if injected else None,
                                 self.entropy.ctypes.data if injected else None)
        dt = time.perf_counter() - t0
        assert rc == 0, rc
        r = np.frombuffer(self.res, dtype=np.int32).reshape(self.n, 4)
        assert not r[:, 0].any() and (r[:, 3] == 168).all(), "stage 1 refused a HELLO"
        self.slots[:] = r[:, 2]
        if injected:
            assert self.reply[:168].tobytes() == self.welcome0, "WELCOME 0 differs from the model's"
        return dt

    def stage2(self, L, acc):
        t0 = time.perf_counter()
        rc = L.cz_acceptor_initiate(acc, self.n, self.slots.ctypes.data, self.init.ctypes.data, self.init.nbytes,
                                    self.ioff.ctypes.data, self.isz.ctypes.data, self.reply.ctypes.data, 288, self.res)
        dt = time.perf_counter() - t0
        assert rc == 0, rc
        r = np.frombuffer(self.res, dtype=np.int32).reshape(self.n, 4)
        assert not r[:, 0].any() and (r[:, 3] == r[0, 3]).all() and r[0, 3] > 30, "stage 2 refused an INITIATE"
        return dt

    def release(self, L, acc):
        for s in self.slots.tolist():
            L.cz_acceptor_release(acc, s)
        assert L.cz_acceptor_pending(acc) == 0


def serial_baseline(pool, reps):
    """64 cz_hs servers, one after another, constructor through READY; seconds per round"""
    from jeromq_amd import handshake
    times = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        for c in pool:
            srv = handshake.CurveServerHandshake(SERVER_SEC, ephemeral_secret=c["seph"], entropy=c["entropy"])
            assert srv.processHandshakeCommand(c["hello"]) == 0
            rc, w = srv.nextHandshakeCommand()
            assert srv.processHandshakeCommand(c["initiate"]) == 0
            rc, r = srv.nextHandshakeCommand()
            assert rc == 0 and srv.status() == handshake.Status.READY
            srv.close()
        times.append(time.perf_counter() - t0)
        assert w.data == pool[-1]["welcome"]
    return times[1:]


def make_client_pool():
    """POOL connections of one client (pool[0]'s long-term pair) to the one server"""
    import hs_model as M
    pool = make_pool()
    cpub, csec = pool[0]["cpub"], pool[0]["csec"]
    for c in pool:
        c["initiate"] = M.client_initiate(c["welcome"], cpub, csec, SERVER_PUB, c["ceph"], c["vnonce"])
        _, state = M.server_welcome(c["hello"], SERVER_SEC, c["seph"], c["entropy"])
        c["ready"], _ = M.server_ready(c["initiate"], state)
    return pool, cpub, csec


class ClientBatch:
    """prebuilt arguments of the three connector stage calls for n connections"""

    def __init__(self, pool, n):
        from jeromq_amd import _lib
        self.n = n
        idx = np.arange(n) % POOL

        def rows(key, width):
            return np.frombuffer(b"".join(c[key] for c in pool), dtype=np.uint8).reshape(POOL, width)[idx].copy()

        self.rsize = len(pool[0]["ready"])
        assert all(len(c["ready"]) == self.rsize for c in pool)
        self.keys = np.frombuffer(SERVER_PUB * n, dtype=np.uint8).copy()
        self.secrets, self.vnonces = rows("ceph", 32), rows("vnonce", 16)
        self.welcomes, self.readys = rows("welcome", 168), rows("ready", self.rsize)
        self.woff = np.arange(n, dtype=np.uint64) * np.uint64(168)
        self.wsize = np.full(n, 168, dtype=np.uint32)
        self.roff = np.arange(n, dtype=np.uint64) * np.uint64(self.rsize)
        self.rsz = np.full(n, self.rsize, dtype=np.uint32)
        self.res = (_lib.cz_accept_result * n)()
        self.reply = np.zeros(n * 513, dtype=np.uint8)
        self.slots = np.zeros(n, dtype=np.int32)
        self.hello0, self.initiate0 = pool[0]["hello"], pool[0]["initiate"]

    def _results(self, reply_len, what):
        r = np.frombuffer(self.res, dtype=np.int32).reshape(self.n, 4)
        assert not r[:, 0].any() and not r[:, 1].any() and (r[:, 3] == reply_len).all(), what
        return r

    def hello(self, L, con, injected=True):
        t0 = time.perf_counter()
        rc = L.cz_connector_hello(con, self.n, self.keys.ctypes.data, self.reply.ctypes.data, 200, self.res,
                                  self.secrets.ctypes.data if injected else None)
        dt = time.perf_counter() - t0
        assert rc == 0, rc
        self.slots[:] = self._results(200, "stage 1 gave no HELLO")[:, 2]
        if injected:
            assert self.reply[:200].tobytes() == self.hello0, "HELLO 0 differs from the model's"
        return dt

    def welcome(self, L, con):
        t0 = time.perf_counter()
        rc = L.cz_connector_welcome(con, self.n, self.slots.ctypes.data, self.welcomes.ctypes.data, self.welcomes.nbytes,
                                    self.woff.ctypes.data, self.wsize.ctypes.data, self.reply.ctypes.data, 513, self.res,
                                    self.vnonces.ctypes.data)
        dt = time.perf_counter() - t0
        assert rc == 0, rc
        self._results(len(self.initiate0), "stage 2 refused a WELCOME")
        assert self.reply[:len(self.initiate0)].tobytes() == self.initiate0, "INITIATE 0 differs from the model's"
        return dt

    def ready(self, L, con):
        t0 = time.perf_counter()
        rc = L.cz_connector_ready(con, self.n, self.slots.ctypes.data, self.readys.ctypes.data, self.readys.nbytes,
                                  self.roff.ctypes.data, self.rsz.ctypes.data, self.res)
        dt = time.perf_counter() - t0
        assert rc == 0, rc
        self._results(0, "stage 3 refused a READY")
        return dt

    def release(self, L, con):
        for s in self.slots.tolist():
            L.cz_connector_release(con, s)
        assert L.cz_connector_pending(con) == 0


def serial_client_baseline(pool, cpub, csec, reps):
    """64 cz_hs clients, one after another, constructor through READY; seconds per round"""
    from jeromq_amd import handshake
    times = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        for c in pool:
            cli = handshake.CurveClientHandshake(cpub, csec, SERVER_PUB, ephemeral_secret=c["ceph"], entropy=c["vnonce"])
            rc, h = cli.nextHandshakeCommand()
            assert cli.processHandshakeCommand(c["welcome"]) == 0
            rc, ini = cli.nextHandshakeCommand()
            assert cli.processHandshakeCommand(c["ready"]) == 0 and cli.status() == handshake.Status.READY
            cli.close()
        times.append(time.perf_counter() - t0)
        assert ini.data == pool[-1]["initiate"]
    return times[1:]


def client_main(args):
    import torch
    from jeromq_amd import _lib
    assert torch.cuda.is_available(), "hs_bench needs a GPU"
    L = _lib.lib()
    pool, cpub, csec = make_client_pool()
    out = {"device": torch.cuda.get_device_name(0), "side": "client", "reps": args.reps, "pool": POOL,
           "clock": "time.perf_counter", "initiate_bytes": len(pool[0]["initiate"]), "batched": []}
    base = serial_client_baseline(pool, cpub, csec, args.reps)
    out["serial_cz_hs"] = {"connections": POOL, "round_ms": [round(t * 1e3, 3) for t in base],
                           "median_round_ms": round(statistics.median(base) * 1e3, 3),
                           "median_per_connection_ms": round(statistics.median(base) * 1e3 / POOL, 4)}
    for n in args.sizes:
        con = ctypes.c_void_p()
        _lib.check(L.cz_connector_create(ctypes.byref(con), cpub, csec, 0, None, 0, n, 0), "cz_connector_create")
        b = ClientBatch(pool, n)
        t1, t2, t3, t1r = [], [], [], []
        for rep in range(args.reps + 1):   # round 0 warms up (buffers grow, code objects load)
            a = b.hello(L, con)
            w = b.welcome(L, con)
            r = b.ready(L, con)
            b.release(L, con)
            g = b.hello(L, con, injected=False)
            b.release(L, con)
            if rep:
                t1.append(a)
                t2.append(w)
                t3.append(r)
                t1r.append(g)
        L.cz_connector_destroy(con)
        ms = lambda v: round(statistics.median(v) * 1e3, 4)  # noqa: E731
        row = {"n": n, "hello_ms": ms(t1), "welcome_ms": ms(t2), "ready_ms": ms(t3), "hello_getrandom_ms": ms(t1r),
               "hello_all_ms": [round(t * 1e3, 4) for t in t1], "welcome_all_ms": [round(t * 1e3, 4) for t in t2],
               "ready_all_ms": [round(t * 1e3, 4) for t in t3],
               "per_connection_us": round(sum(statistics.median(t) for t in (t1, t2, t3)) * 1e6 / n, 3)}
        out["batched"].append(row)
        print(f"n={n}: hello {row['hello_ms']} ms, welcome {row['welcome_ms']} ms, ready {row['ready_ms']} ms",
              file=sys.stderr)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


HANDOVER_SIZES = (64, 1024, 16384, 65536)
# what "--handover" was written to find out, fixed before the first run; each is marked from the run
HANDOVER_HYPOTHESES = (
    ("batch_10x_from_1024", "(b) the bulk add + release is at least 10x below (a) the per-slot loop from N = 1024"),
    ("handover_minor_share", "after the change the hand-over (b) is a minor share of a storm: at most a quarter of "
                             "stage 1 + stage 2 at every N"),
)


def handover_main(args):
    """The last step of a storm: N accepted sessions into the engine and out of the acceptor's table, and
    out of the engine again.  Per round, for each N, both ways in turn (which goes first alternates):
      (a) loop of cz_engine_add_accepted + cz_acceptor_release   | (b) cz_engine_add_accepted_batch + cz_acceptor_release_batch
      (c) loop of cz_engine_remove_conn                           |     cz_engine_remove_conns
    each behind its own stage 1 + stage 2 (timed, (d)), on its own engine so that both see the same
    history; round 0 warms up (tables and staging grow), then the median of --reps rounds."""
    import torch
    from jeromq_amd import _lib
    assert torch.cuda.is_available(), "hs_bench needs a GPU"
    L = _lib.lib()
    pool = make_pool()
    out = {"device": torch.cuda.get_device_name(0), "what": "handover", "reps": args.reps, "pool": POOL,
           "clock": "time.perf_counter", "rows": []}
    for n in args.sizes:
        acc = ctypes.c_void_p()
        _lib.check(L.cz_acceptor_create(ctypes.byref(acc), SERVER_SEC, 0, None, 0, n, 0), "cz_acceptor_create")
        engines = {}
        for leg in ("loop", "batch"):
            h = ctypes.c_void_p()
            _lib.check(L.cz_engine_create(ctypes.byref(h), 4096, 0), "cz_engine_create")
            engines[leg] = h
        b = Batch(pool, n)
        ids = np.zeros(n, dtype=np.int32)
        rcs = np.zeros(n, dtype=np.int32)
        t = {k: [] for k in ("stage1", "stage2", "loop_add", "batch_add", "loop_remove", "batch_remove")}

        def loop_leg(eng):
            slots = b.slots.tolist()
            t0 = time.perf_counter()
            got = [L.cz_engine_add_accepted(eng, acc, s) for s in slots]
            for s in slots:
                L.cz_acceptor_release(acc, s)
            t1 = time.perf_counter()
            assert min(got) >= 0 and L.cz_acceptor_pending(acc) == 0
            t2 = time.perf_counter()
            bad = sum(L.cz_engine_remove_conn(eng, c) for c in got)
            t3 = time.perf_counter()
            assert bad == 0
            return t1 - t0, t3 - t2

        def batch_leg(eng):
            t0 = time.perf_counter()
            rc1 = L.cz_engine_add_accepted_batch(eng, acc, n, b.slots.ctypes.data, ids.ctypes.data)
            rc2 = L.cz_acceptor_release_batch(acc, n, b.slots.ctypes.data)
            t1 = time.perf_counter()
            assert rc1 == 0 and rc2 == 0 and ids.min() >= 0 and L.cz_acceptor_pending(acc) == 0
            t2 = time.perf_counter()
            rc3 = L.cz_engine_remove_conns(eng, n, ids.ctypes.data, rcs.ctypes.data)
            t3 = time.perf_counter()
            assert rc3 == 0 and not rcs.any()
            return t1 - t0, t3 - t2

        for rep in range(args.reps + 1):
            order = ("loop", "batch") if rep % 2 else ("batch", "loop")
            for leg in order:
                s1 = b.stage1(L, acc)
                s2 = b.stage2(L, acc)
                add, rem = (loop_leg if leg == "loop" else batch_leg)(engines[leg])
                if rep:
                    t["stage1"].append(s1)
                    t["stage2"].append(s2)
                    t[leg + "_add"].append(add)
                    t[leg + "_remove"].append(rem)
        for h in engines.values():
            L.cz_engine_destroy(h)
        L.cz_acceptor_destroy(acc)
        med = {k: statistics.median(v) * 1e3 for k, v in t.items()}
        hs = med["stage1"] + med["stage2"]
        row = {"n": n, "stage1_ms": round(med["stage1"], 4), "stage2_ms": round(med["stage2"], 4),
               "loop_add_release_ms": round(med["loop_add"], 4), "batch_add_release_ms": round(med["batch_add"], 4),
               "loop_remove_ms": round(med["loop_remove"], 4), "batch_remove_ms": round(med["batch_remove"], 4),
               "add_release_speedup": round(med["loop_add"] / med["batch_add"], 2),
               "remove_speedup": round(med["loop_remove"] / med["batch_remove"], 2),
               "handover_over_handshake_before": round(med["loop_add"] / hs, 4),
               "handover_over_handshake_after": round(med["batch_add"] / hs, 4),
               "all_ms": {k: [round(x * 1e3, 4) for x in v] for k, v in t.items()}}
        out["rows"].append(row)
        print(f"n={n}: stages {hs:.3f} ms; add+release loop {med['loop_add']:.3f} ms, bulk {med['batch_add']:.3f} ms; "
              f"remove loop {med['loop_remove']:.3f} ms, bulk {med['batch_remove']:.3f} ms", file=sys.stderr)
    verdicts = {
        "batch_10x_from_1024": all(r["add_release_speedup"] >= 10 for r in out["rows"] if r["n"] >= 1024),
        "handover_minor_share": all(r["handover_over_handshake_after"] <= 0.25 for r in out["rows"]),
    }
    out["hypotheses"] = [{"id": k, "statement": s, "verdict": "confirmed" if verdicts[k] else "contradicted"}
                         for k, s in HANDOVER_HYPOTHESES]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--side", choices=("server", "client"), default="server")
    ap.add_argument("--handover", action="store_true",
                    help="time the session hand-over (acceptor -> engine -> gone), per slot against bulk, beside the "
                         "two handshake stages; N = 64, 1024, 16384, 65536, median of 7; writes hs_handover.json")
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--sizes", type=int, nargs="*", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 7 if args.handover else 5
    if args.sizes is None:
        args.sizes = list(HANDOVER_SIZES if args.handover else SIZES)
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if args.handover:
        if args.out is None:
            args.out = os.path.join(ROOT, "profiles", "hs_batch", "hs_handover.json")
        return handover_main(args)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "hs_batch",
                                "hs_connect.json" if args.side == "client" else "hs_batch.json")
    if args.side == "client":
        return client_main(args)
    import torch
    from jeromq_amd import _lib
    assert torch.cuda.is_available(), "hs_bench needs a GPU"
    L = _lib.lib()
    pool = make_pool()
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "pool": POOL, "clock": "time.perf_counter",
           "initiate_bytes": len(pool[0]["initiate"]), "batched": []}
    base = serial_baseline(pool, args.reps)
    out["serial_cz_hs"] = {"connections": POOL, "round_ms": [round(t * 1e3, 3) for t in base],
                           "median_round_ms": round(statistics.median(base) * 1e3, 3),
                           "median_per_connection_ms": round(statistics.median(base) * 1e3 / POOL, 4)}
    for n in args.sizes:
        acc = ctypes.c_void_p()
        _lib.check(L.cz_acceptor_create(ctypes.byref(acc), SERVER_SEC, 0, None, 0, n, 0), "cz_acceptor_create")
        b = Batch(pool, n)
        t1, t2, t1r = [], [], []
        for rep in range(args.reps + 1):   # round 0 warms up (buffers grow, code objects load)
            a = b.stage1(L, acc)
            c = b.stage2(L, acc)
            b.release(L, acc)
            r = b.stage1(L, acc, injected=False)
            b.release(L, acc)
            if rep:
                t1.append(a)
                t2.append(c)
                t1r.append(r)
        L.cz_acceptor_destroy(acc)
        ms = lambda v: round(statistics.median(v) * 1e3, 4)  # noqa: E731
        row = {"n": n, "stage1_ms": ms(t1), "stage2_ms": ms(t2), "stage1_getrandom_ms": ms(t1r),
               "stage1_all_ms": [round(t * 1e3, 4) for t in t1], "stage2_all_ms": [round(t * 1e3, 4) for t in t2],
               "per_connection_us": round((statistics.median(t1) + statistics.median(t2)) * 1e6 / n, 3)}
        out["batched"].append(row)
        print(f"n={n}: stage 1 {row['stage1_ms']} ms, stage 2 {row['stage2_ms']} ms", file=sys.stderr)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
