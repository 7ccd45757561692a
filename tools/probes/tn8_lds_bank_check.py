#!/usr/bin/env python3
"""LDS bank-conflict degree of every fragment read of gemm_tn8_kernel (csrc/gemm.hip), both MFMA flavours, on the CPU.

A half-tile is 64 reduction rows x 128 columns of 16-bit elements (256-byte rows, sixteen 16-byte chunks per row).  The staging DMA writes it
lane-linear and permutes on the SOURCE side, so chunk ch of row r lands at position image(r, ch) of the row:
    MSHAPE 32:  ch ^ 4 (r & 3)
    MSHAPE 16:  ch ^ (((r & 3) << 2) | (((r >> 3) & 1) << 1))
A fragment is two ds_read_b64_tr_b16 (rows +0..3 and +4..7 of an 8-row group).  Per 16-lane group, lane 4q + p supplies the address of the four
elements 4p .. 4p+3 of row q of a 4-row x 16-column block.  The 32x32x16 operand takes, per 32-lane half, two blocks side by side (32 columns of the
same rows); the 16x16x32 operand takes two blocks of the SAME 16 columns 8 rows apart.

Bank rule (ds_read_b64_tr_b16 = ds_read_b64): the wave is served in two groups of 32 lanes; the bank of byte address a is (a / 4) mod 64; identical
dwords broadcast; every further distinct dword on a busy bank adds one cycle.  degree = the largest number of distinct dwords on one bank.

The MSHAPE 16 image moves row bit 3 (the two blocks of a 32-lane half) into chunk bit 1 and leaves row bit 2 alone, so that the second read of a
fragment (+4 rows) stays at offset:1024 from the first in every lane: an image that swizzles with (r >> 2) & 3 needs a second address there.

The script also replays the staging and every read on a numbered tile, so that a wrong address (the second read's delta, say) shows as a wrong
element here and not as a wrong gradient on the device.

    python tools/probes/tn8_lds_bank_check.py
"""
import sys

ROW_BYTES = 256


def image(mshape, row, ch):
    if mshape == 32:
        return ch ^ (4 * (row & 3))
    return ch ^ (((row & 3) << 2) | (((row >> 3) & 1) << 1))


def staged_half(mshape):
    """LDS bytes offset -> (row, first column) of the 8 bytes (4 elements) stored there, as the staging stream of the kernel writes a half-tile:
    wave w, piece i: rows 4 (2w + i) + (lane >> 4), LDS side lane-linear, source chunk = the inverse image (the XOR is its own inverse)."""
    lds = {}
    for wave in range(8):
        for i in range(2):
            for lane in range(64):
                lrow, lch = lane >> 4, lane & 15
                row = (wave * 2 + i) * 4 + lrow
                src_ch = image(mshape, row, lch)                      # logical chunk whose bytes this lane fetches
                off = wave * 2048 + i * 1024 + lane * 16
                assert off == row * ROW_BYTES + lch * 16
                lds[off] = (row, src_ch * 8)
                lds[off + 8] = (row, src_ch * 8 + 4)
    return lds


def fragment_reads(mshape, operand, who, blk, ks):
    """The two reads of one fragment -> [(64 lane byte offsets inside the half, 64 expected (row, first column))] as the kernel addresses them.
    operand 'z': who = wave row (0..1), 64 columns per half; 'x': who = wave column (0..3), 32 columns per half."""
    col0 = who * 64 if operand == "z" else who * 32
    out = []
    for second in range(2):
        addrs, want = [], []
        for lane in range(64):
            g4, pl = lane >> 4, lane & 15
            prow, fsub = pl >> 2, (pl & 1) << 3
            if mshape == 32:
                row = ks * 16 + 8 * (g4 >> 1) + prow
                ch = ((col0 + blk * 32 + 16 * (g4 & 1)) >> 3) + ((pl & 3) >> 1)
                a = row * ROW_BYTES + ((ch ^ (4 * prow)) << 4) + fsub + 1024 * second           # one base, offset:1024
            else:
                row = ks * 32 + 8 * g4 + prow
                ch = ((col0 + blk * 16) >> 3) + ((pl & 3) >> 1)
                a = row * ROW_BYTES + ((ch ^ ((prow << 2) | ((g4 & 1) << 1))) << 4) + fsub + 1024 * second   # (the image leaves row bit 2 alone)
            addrs.append(a)
            want.append((row + 4 * second, ch * 8 + 4 * (pl & 1)))
        out.append((addrs, want))
    return out


def conflict_degree(addrs):
    worst = 1
    for half in (addrs[:32], addrs[32:]):
        banks = {}
        for a in half:
            for dw in (a // 4, a // 4 + 1):
                banks.setdefault(dw % 64, set()).add(dw)
        worst = max(worst, max(len(s) for s in banks.values()))
    return worst


def all_fragments(mshape):
    nb_z, nb_x, steps = (2, 1, 4) if mshape == 32 else (4, 2, 2)
    for operand, whos, nb in (("z", 2, nb_z), ("x", 4, nb_x)):
        for who in range(whos):
            for blk in range(nb):
                for ks in range(steps):
                    yield operand, who, blk, ks


def check(mshape):
    """-> (worst conflict degree over every fragment read, number of reads, number of lanes that would receive a wrong element)"""
    lds = staged_half(mshape)
    worst, n, wrong = 1, 0, 0
    for operand, who, blk, ks in all_fragments(mshape):
        for addrs, want in fragment_reads(mshape, operand, who, blk, ks):
            worst = max(worst, conflict_degree(addrs))
            n += 1
            wrong += sum(1 for a, w in zip(addrs, want) if lds.get(a) != w)
    return worst, n, wrong


def naive_16_on_32_image():
    """the 16x16x32 read pattern on the MSHAPE 32 image (what the flavour would cost without its own image)"""
    worst = 1
    for operand, who, blk, ks in all_fragments(16):
        col0 = who * 64 if operand == "z" else who * 32
        for second in range(2):
            addrs = []
            for lane in range(64):
                g4, pl = lane >> 4, lane & 15
                prow = pl >> 2
                row = ks * 32 + 8 * g4 + prow + 4 * second
                ch = ((col0 + blk * 16) >> 3) + ((pl & 3) >> 1)
                addrs.append(row * ROW_BYTES + (image(32, row, ch) << 4) + ((pl & 1) << 3))
            worst = max(worst, conflict_degree(addrs))
    return worst


def main():
    ok = True
    for mshape in (32, 16):
        worst, n, wrong = check(mshape)
        print(f"MSHAPE {mshape}: {n} fragment reads (ds_read_b64_tr_b16) over all wave rows / columns, worst conflict degree {worst}-way, {wrong} wrong elements")
        ok = ok and worst == 1 and wrong == 0
    print(f"16x16x32 read pattern on the MSHAPE 32 image: {naive_16_on_32_image()}-way")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
