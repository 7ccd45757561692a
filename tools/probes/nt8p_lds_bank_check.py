#!/usr/bin/env python3
"""LDS addressing of gemm_nt8p_kernel (csrc/gemm.hip), both MFMA flavours, replayed on the CPU: every fragment read of the k-loop and the
epilogue units' slab writes and read-backs, on a numbered tile, with the bank-conflict degree of each instruction.

Half-tiles.  A half is 128 rows x 64 k of 16-bit elements (128-byte rows, eight 16-byte chunks).  The staging DMA writes it lane-linear and
permutes on the SOURCE side: LDS row lr, position s holds logical chunk s ^ ((lr >> 1) & 7).  Rows 64 wr + 32 i2 .. + 31 of an A half are the
32-row block i2 of wave row wr; rows 32 wc .. + 31 of a B half are wave column wc's 32 output columns.
Fragments (one ds_read_b128 each, four per 32-row block and k-tile in either flavour):
    MSHAPE 32 (32 x 32 x 16): step ks = 0..3, lane l reads row l & 31, chunk 2 ks + (l >> 5)             = k 16 ks + 8 (l >> 5) .. + 7
    MSHAPE 16 (16 x 16 x 32): sub-block s, step ks' = 0..1, lane l reads row 16 s + (l & 15), chunk 4 ks' + (l >> 4) = k 32 ks' + 8 (l >> 4) .. + 7
Slab (one 32-row unit of the wave tile, 32 rows x 64 columns of 16-bit outputs, 128-byte rows): column chunk c of row r sits at position
c ^ (r & 7).  Writes are 8 bytes (four outputs of one row), read-backs 16 bytes (row 8 it + (l >> 3), chunk l & 7):
    MSHAPE 32: register quad q of block jj: row l & 31, columns 32 jj + 8 q + 4 (l >> 5) .. + 3
    MSHAPE 16: quad (ms, ns) of block jj:   row 16 ms + (l & 15), columns 32 jj + 16 ns + 4 (l >> 4) .. + 3

Bank rules (MI355X_MICROARCH.md, LDS): a wave64 access is served in fixed lane groups, one LDS cycle per group when conflict-free; identical
dwords broadcast; every further distinct dword on a busy bank of a group adds a cycle, degree = the largest number of distinct dwords on one bank.
    ds_read_b128: four groups of 16 lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, {32-35, 44-47, 52-59}, {36-43, 48-51, 60-63};
                  bank of byte address a = (a / 4) mod 64
    ds_write_b64: four groups of 16 contiguous lanes; bank = (a / 4) mod 32

    python tools/probes/nt8p_lds_bank_check.py
"""
import sys

ROW = 128
READ_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
READ_GROUPS += [[l + 32 for l in g] for g in READ_GROUPS]
WRITE_GROUPS = [list(range(16 * g, 16 * g + 16)) for g in range(4)]


def degree(addrs, groups, dwords, banks):
    worst = 1
    for g in groups:
        busy = {}
        for l in g:
            for d in range(dwords):
                dw = addrs[l] // 4 + d
                busy.setdefault(dw % banks, set()).add(dw)
        worst = max(worst, max(len(s) for s in busy.values()))
    return worst


def staged_half():
    """LDS byte offset inside a half -> (LDS row, first k) of the 16 bytes the staging stream puts there (wave w, piece i, lane)"""
    lds = {}
    for wave in range(8):
        for i in range(2):
            for lane in range(64):
                lrow, lsc = lane >> 3, lane & 7
                lr = (wave * 2 + i) * 8 + lrow
                c = lsc ^ ((lr >> 1) & 7)                           # the source chunk this lane fetches
                off = wave * 2048 + i * 1024 + lane * 16
                assert off == lr * ROW + lsc * 16
                lds[off] = (lr, c * 8)
    return lds


def fragment_reads(mshape):
    """every fragment read of one k-tile -> (64 byte offsets inside the half, 64 expected (row, first k)); base = 64 wr + 32 i2 (A) or 32 wc (B):
    every 32-row block of the half"""
    for base in range(0, 128, 32):
        for f in range(4):
            addrs, want = [], []
            for lane in range(64):
                if mshape == 32:
                    row, ch = lane & 31, 2 * f + (lane >> 5)
                    sw = ((lane & 31) >> 1) & 7
                else:
                    sub, ks = f >> 1, f & 1
                    row, ch = 16 * sub + (lane & 15), 4 * ks + (lane >> 4)
                    sw = ((lane & 15) >> 1) & 7
                addrs.append(base * ROW + row * ROW + ((ch ^ sw) << 4))
                want.append((base + row, ch * 8))
            yield addrs, want


def slab_writes(mshape):
    """the eight 8-byte writes of a unit -> (64 byte offsets inside the slab, 64 (row, first column))"""
    for c in range(8):
        addrs, what = [], []
        for lane in range(64):
            if mshape == 32:
                row, hi = lane & 31, lane >> 5
                addrs.append(row * ROW + ((c ^ (row & 7)) << 4) + 8 * hi)
                what.append((row, 8 * c + 4 * hi))
            else:
                jj, ms, ns = c >> 2, (c >> 1) & 1, c & 1
                row, g4 = 16 * ms + (lane & 15), lane >> 4
                ch = 4 * jj + 2 * ns + (g4 >> 1)
                addrs.append(row * ROW + ((ch ^ (row & 7)) << 4) + 8 * (g4 & 1))
                what.append((row, 32 * jj + 16 * ns + 4 * g4))
        yield addrs, what


def slab_readbacks():
    for it in range(4):
        addrs, want = [], []
        for lane in range(64):
            prow, pch = lane >> 3, lane & 7
            row = it * 8 + prow
            addrs.append(row * ROW + ((pch ^ (row & 7)) << 4))
            want.append((row, 8 * pch))
        yield addrs, want


def check(mshape):
    """-> dict: worst conflict degree of the fragment reads / slab writes / read-backs, their counts, and the number of wrong elements"""
    lds = staged_half()
    res = {"frag_worst": 1, "frag_reads": 0, "write_worst": 1, "writes": 0, "readback_worst": 1, "readbacks": 0, "wrong": 0}
    for addrs, want in fragment_reads(mshape):
        res["frag_worst"] = max(res["frag_worst"], degree(addrs, READ_GROUPS, 4, 64))
        res["frag_reads"] += 1
        res["wrong"] += sum(1 for a, w in zip(addrs, want) if lds.get(a) != w)
    slab = {}
    for addrs, what in slab_writes(mshape):
        res["write_worst"] = max(res["write_worst"], degree(addrs, WRITE_GROUPS, 2, 32))
        res["writes"] += 1
        for a, w in zip(addrs, what):
            assert a not in slab, "two lanes write the same 8 bytes"
            slab[a] = w
    res["wrong"] += 32 * 16 - len(slab)                              # every 8 bytes of the 4 KiB slab written exactly once
    for addrs, want in slab_readbacks():
        res["readback_worst"] = max(res["readback_worst"], degree(addrs, READ_GROUPS, 4, 64))
        res["readbacks"] += 1
        for a, (row, col) in zip(addrs, want):
            res["wrong"] += slab.get(a) != (row, col)
            res["wrong"] += slab.get(a + 8) != (row, col + 4)
    return res


def main():
    r = {m: check(m) for m in (32, 16)}
    for m in (32, 16):
        v = r[m]
        print(f"MSHAPE {m}: {v['frag_reads']} fragment reads (ds_read_b128) worst {v['frag_worst']}-way | {v['writes']} slab writes (ds_write_b64) worst "
              f"{v['write_worst']}-way | {v['readbacks']} read-backs (ds_read_b128) worst {v['readback_worst']}-way | {v['wrong']} wrong elements")
    ok = all(v["wrong"] == 0 for v in r.values())
    ok = ok and all(r[16][k] <= r[32][k] for k in ("frag_worst", "write_worst", "readback_worst"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
