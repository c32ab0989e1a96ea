"""The headline seal's pair loop, counted in the shipped machine code (CPU: reads the product
library's gfx950 code object).

k_seal_uniform<1, true, 0> spends its time in the steady pair loop of seal_frame (cz_kernels.hip):
one 128-byte payload line in (8 global_load_dwordx4), two Salsa20 blocks, eight Poly1305 blocks, one
128-byte body line out (8 buffer_store_dwordx4).  The kernel is VALU-issue-bound and every int32
VALU instruction costs its SIMD 4 cycles, so the loop's `v_` count is its
cost.  The loop is found as the backward branch whose body holds those 8 loads and 8 stores (a
whole number of times, should the loop ever run several pairs per trip: the counts are per pair);
the count per pair must not grow past what the loop was brought down to, and the register copies
and selects that were removed from it (64-bit moves under conditional loads, a select per
Poly1305 block) must not come back.

The loop before this test was written, counted by the same functions: 1927 VALU per pair, with 8
v_mov_b64 and 7 v_cndmask_b32."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "k_seal_uniformILi1ELb1ELi0E"
PAIR_LOOP_VALU_MAX = 1920       # the headline's loop, per pair (before: 1927)
PAIR_LOOP_VALU_MAX_ANY = 1942   # the per-lane-rounds copy of it (before: 1949)

_INS = re.compile(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):")
_TARGET = re.compile(r"<[^>+]+\+0x([0-9a-fA-F]+)>\s*$")


def kernel_instructions(lib, kernel=KERNEL):
    """[(address, opcode, branch target address or None)] of `kernel` in `lib`'s gfx950 code"""
    from jeromq_amd import build
    for co in build.device_code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            text = subprocess.run([os.path.join(build.LLVM_BIN, "llvm-objdump"), "-d", f"--mcpu={build.ARCH}", f.name],
                                  check=True, capture_output=True, text=True).stdout
        if kernel not in text:
            continue
        out, base, inside = [], None, False
        for ln in text.splitlines():
            head = re.match(r"^([0-9a-fA-F]+) <(.*)>:$", ln)
            if head:
                inside = kernel in head.group(2)
                base = int(head.group(1), 16)
                continue
            if not inside:
                continue
            m = _INS.match(ln)
            if not m:
                continue
            tgt = _TARGET.search(ln) if m.group(1).startswith(("s_cbranch", "s_branch")) else None
            out.append((int(m.group(3), 16), m.group(1), base + int(tgt.group(1), 16) if tgt else None))
        if out:
            return out
    return []


def pair_loops(ins):
    """(pairs per trip, opcodes, code bytes) of the loops made of whole pairs -- 8 line loads and 8 line
    stores each: the span of a backward branch"""
    addr = {a: i for i, (a, _, _) in enumerate(ins)}
    found = []
    for i, (a, op, tgt) in enumerate(ins):
        if tgt is None or tgt > a or tgt not in addr:
            continue
        body = [o for _, o, _ in ins[addr[tgt]:i + 1]]
        n = body.count("global_load_dwordx4")
        if n and n % 8 == 0 and body.count("buffer_store_dwordx4") == n:
            found.append((n // 8, body, a + 8 - tgt))
    return found


def valu(body):
    return sum(1 for o in body if o.startswith("v_"))


@pytest.fixture(scope="module")
def loops():
    from jeromq_amd import build
    if not os.path.exists(build.PRODUCT_LIB):
        pytest.skip("library not built")
    ins = kernel_instructions(build.PRODUCT_LIB)
    assert ins, f"{KERNEL} not found in the library"
    found = pair_loops(ins)
    assert found, "no loop of whole pairs (8 global_load_dwordx4 and 8 buffer_store_dwordx4 each) found"
    return found


def test_pair_loop_valu_count(loops):
    """the kernel holds the loop twice, for waves whose high nonce word is wave-uniform (rounds 1-2
    partly on the scalar unit: the headline's loop, the cheaper one) and for waves that straddle a
    change of it"""
    per_pair = sorted(valu(body) / pairs for pairs, body, _ in loops)
    print(f"pair loops: VALU per pair {per_pair}, pairs per trip {[p for p, _, _ in loops]}")
    assert per_pair[0] <= PAIR_LOOP_VALU_MAX, f"{per_pair[0]} VALU per pair, the loop was at {PAIR_LOOP_VALU_MAX}"
    assert per_pair[-1] <= PAIR_LOOP_VALU_MAX_ANY


def test_pair_loop_has_no_selects_or_wide_moves(loops):
    for _, body, _ in loops:
        bad = [o for o in body if o.startswith(("v_cndmask", "v_mov_b64"))]
        assert not bad, f"{len(bad)} select / 64-bit move instructions in a pair loop: {sorted(set(bad))}"


def test_pair_loop_fits_the_instruction_cache(loops):
    """the loop stays under 32 KiB of code (two pairs per trip measured slower at 29 KiB: DESIGN.md section 6)"""
    for _, _, size in loops:
        assert size < 32 * 1024, f"pair loop of {size} bytes"
