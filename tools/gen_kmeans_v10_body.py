#!/usr/bin/env python3
"""Generate ``alink_amd/ops/csrc/kmeans_v10_body.h``: the VALU accumulate of kmeans_v10.hip as ONE inline-asm block per
tile pair (``KM10_ACC_PAIR``: 2 x 16 rows per accumulate wave; GPR-indexed adds into the register-resident sums
v[32:255]).

Accumulate wave a owns the 16 rows r = 16q + 4a + m (q, m = 0..3) of every 64-row tile: their X-tile swizzle
``xsw(r) = 4m + a`` takes only four values, so the four lane addresses (one per m, v[12:15]) are computed once
per tile and row (q, m) is read at ``v[12+m] + (16q + m) * 256``.  Lane l owns dims 2l, 2l+1 (v[32+2c] / v[33+2c]):
one dword per row brings both bf16 values, and ``v_dot2_f32_bf16`` with the packed constants (1, 0) / (0, 1) adds the
low / high value into its accumulator (src2 and dst GPR-indexed): 2 VALU per row.

GPR-indexing mode is switched on ONCE per pair.  The distance waves publish every row's id as a ready-made 16-bit
M0 image, ``0xC000 | 2c`` (index in bits 7:0, the SRC2 | DST mode bits in 15:12), two rows per dword (row 4q + m in
half m & 1 of word 2q + m / 2): the index moves with ONE SALU write of M0 per row, ``s_mov_b32`` for the low half
(the other row's image in bits 31:16 is ignored by the index logic) and ``s_lshr_b32 .. 16`` for the high half.
``s_set_gpr_idx_on`` takes the first row's index from its word itself.

The block:
  * the 16 id words of the pair are ONE ``ds_read_b32`` (lane i < 16 reads word i) and 16 ``v_readlane_b32``, issued
    ahead of tile A's row reads and waited for only after them: one LDS round trip for the ids and the first rows;
  * rows come in pairs 4,096 B apart on one address register: ``ds_read2st64_b32`` (offsets in units of 256 B), the
    rows (q, m), (q + 1, m) per read into an even/odd register pair, 8 reads per tile;
  * rolling refill: as soon as a half of tile A (8 rows, registers v16..v23 or v24..v31) has been consumed, tile B's
    reads of that half are issued into the registers just freed, BEFORE tile A's next half; tile B's addresses
    replace tile A's in v[12:15] once tile A's reads are issued.  The v_dot2 order is all of A, then all of B, rows
    in the order q, m.
LDS returns in order, so every ``s_waitcnt lgkmcnt`` immediate is static: the emitter keeps the queue of
outstanding reads and derives (and asserts) each count from it.
"""
import os
import sys

ROWS_PER_DWORD = 2
LGKM_MAX = 15          # lgkmcnt is a 4-bit field
# The block's scalars live in FIXED SGPRs, named as clobbers (KM10_ACC_PAIR_CLOBBERS), not as operands: an asm
# statement takes at most 30 operands and the seven accumulator blocks alone are 14.
ID_SGPR = 84           # s84..s99: the pair's 16 id words
KEEP_SGPR = 83          # the saved M0


class Emit:
    """Instruction list plus the in-order queue of outstanding LDS reads (tags), for static lgkmcnt waits."""

    def __init__(self):
        self.lines = []
        self.queue = []
        self.landed = set()

    def op(self, text):
        self.lines.append(text)

    def lds(self, text, tag):
        assert tag not in self.queue and tag not in self.landed, tag
        self.lines.append(text)
        self.queue.append(tag)

    def need(self, tags):
        """Wait until every read in ``tags`` has returned: allow only the reads issued after the newest of them."""
        pend = [i for i, t in enumerate(self.queue) if t in tags]
        assert all(t in self.landed or t in self.queue for t in tags), tags
        if not pend:
            return
        cnt = len(self.queue) - 1 - max(pend)
        cnt = min(cnt, LGKM_MAX)               # a smaller count only waits for more
        self.lines.append(f"s_waitcnt lgkmcnt({cnt})")
        self.landed.update(self.queue[:len(self.queue) - cnt])
        self.queue = self.queue[len(self.queue) - cnt:]

    def use(self, tag):
        assert tag in self.landed, f"read {tag} consumed before its wait"


def _dots(e, reg, tag):
    e.use(tag)
    e.op(f"v_dot2_f32_bf16 v32, v{reg}, %[one_lo], v32")
    e.op(f"v_dot2_f32_bf16 v33, v{reg}, %[one_hi], v33")


def _index(e, word, m, first):
    """M0 for row (q, m) whose id image sits in half m & 1 of ``word``; the block's first row rides on idx_on."""
    if m % ROWS_PER_DWORD:
        e.op(f"s_lshr_b32 m0, {word}, 16")
    elif not first:
        e.op(f"s_mov_b32 m0, {word}")


def _reg(q, m):
    """Register of row (q, m): half h = q / 2 owns v[16 + 8h .. 23 + 8h], the read of pair m lands in 2m, 2m + 1."""
    return 16 + 8 * (q >> 1) + 2 * m + (q & 1)


def _read_half(e, t, h):
    for m in range(4):
        lo = _reg(2 * h, m)
        assert _reg(2 * h + 1, m) == lo + 1 and lo % 2 == 0
        o0, o1 = 16 * (2 * h) + m, 16 * (2 * h + 1) + m           # units of 64 dwords = 256 B = one row
        assert o1 - o0 == 16 and o1 < 256
        e.lds(f"ds_read2st64_b32 v[{lo}:{lo + 1}], v{12 + m} offset0:{o0} offset1:{o1}", (t, h, m))


def _consume_half(e, t, h):
    e.need({(t, h, m) for m in range(4)})
    for q in (2 * h, 2 * h + 1):
        for m in range(4):
            _index(e, f"s{ID_SGPR + 8 * t + 2 * q + m // ROWS_PER_DWORD}", m, t == 0 and q == 0 and m == 0)
            _dots(e, _reg(q, m), (t, h, m))


def _addresses(e, slot):
    e.op(f"v_add_u32 v12, %[{slot}], %[aoff]")
    e.op("v_xor_b32 v13, 64, v12")
    e.op("v_xor_b32 v14, 0x80, v12")
    e.op("v_xor_b32 v15, 0xc0, v12")


def pair_body():
    e = Emit()
    e.lds("ds_read_b32 %[idv], %[idad]", "ids")
    _addresses(e, "slota")
    _read_half(e, 0, 0)
    _read_half(e, 0, 1)
    _addresses(e, "slotb")                  # tile A's reads are issued: v[12:15] are free
    e.op(f"s_mov_b32 s{KEEP_SGPR}, m0")
    e.need({"ids"})
    for i in range(16):
        e.op(f"v_readlane_b32 s{ID_SGPR + i}, %[idv], {i}")
    e.op(f"s_set_gpr_idx_on s{ID_SGPR}, gpr_idx(SRC2,DST)")
    for h in range(2):
        _consume_half(e, 0, h)
        _read_half(e, 1, h)                 # into exactly the registers this half's v_dot2 have just read
    for h in range(2):
        _consume_half(e, 1, h)
    e.op("s_set_gpr_idx_off")
    e.op(f"s_mov_b32 m0, s{KEEP_SGPR}")
    assert not e.queue
    dots = [ln for ln in e.lines if ln.startswith("v_dot2")]
    reads = [ln for ln in e.lines if ln.startswith("ds_read")]
    waits = [ln for ln in e.lines if ln.startswith("s_waitcnt")]
    assert len(dots) == 64 and len(reads) == 17
    assert waits == [f"s_waitcnt lgkmcnt({c})" for c in (8, 4, 4, 4, 0)]
    rows = [int(ln.split(",")[1].strip()[1:]) for ln in dots[0::2]]
    assert rows == 2 * [_reg(q, m) for q in range(4) for m in range(4)]      # all of A, then all of B, rows q, m
    return e.lines


def _macro(name, lines):
    out = [f"#define {name} \\"]
    out += [f'    "{ln}\\n\\t" \\' for ln in lines]
    out.append('    ""')
    return out


def body():
    out = ["// GENERATED by tools/gen_kmeans_v10_body.py -- do not edit", "#pragma once"]
    out += _macro("KM10_ACC_PAIR", pair_body())
    out.append("#define KM10_ACC_PAIR_CLOBBERS " +
               ", ".join(f'"s{r}"' for r in list(range(ID_SGPR, ID_SGPR + 16)) + [KEEP_SGPR]))
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alink_amd", "ops", "csrc",
                       "kmeans_v10_body.h")
    text = body()
    if "--check" in sys.argv:
        sys.exit(0 if open(dst).read() == text else 1)
    open(dst, "w").write(text)
