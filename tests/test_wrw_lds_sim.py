"""CPU replay of conv3x3_wrw_kernel (ops/csrc/wrw_kernels.hip).

No GPU needed. Replayed from the kernel's own index arithmetic:
  * the staging store map of one sub-image: a bijection onto the image;
  * ds_read_b64_tr_b16 (lane 4q+p of a 16-lane group passes the address
    of pixel q, channels 4p..4p+3; lane i receives channel i of the four
    pixels): every pair of reads rebuilds the MFMA operand element
    (channel = lane & 15, pixel = j0 + 8*(lane>>4) + e) for dx = 0, 1, 2;
  * the gfx950 bank rule for that instruction -- bank = (byte / 4) mod
    64, conflicts counted inside each 32-lane half -- asserting no two
    lanes of a half hit one bank at different addresses, and 8-byte
    alignment of every address;
  * the whole walk in float64: slabs, the load-only first step of an
    image, the ring of x rows, column tiles, chunks, the wave split, the
    partial records and the finishing kernel, against autograd.
"""
import os
import re

import pytest
import torch
import torch.nn.functional as F

R = 2
XSLOTS = R + 2
TW_ALL = 384
K_BLOCK = 256

CONFIGS = [(1, 1), (1, 2), (1, 4), (2, 1), (2, 2), (2, 4), (3, 1), (3, 2),
           (4, 1), (4, 2), (4, 4)]


class Cfg:
    """Mirror of the kernel's Cfg<CT, KT>."""

    def __init__(self, CT, KT):
        self.CT, self.KT = CT, KT
        self.TW = TW_ALL // max(CT, KT)
        self.XS = (self.TW + 9) * 32
        self.GS = (self.TW + 1) * 32
        self.XROW = CT * self.XS
        self.GROW = KT * self.GS
        self.X_BYTES = XSLOTS * self.XROW
        self.STAGE_BYTES = self.X_BYTES + R * self.GROW
        self.NWC = 1 if CT == 3 else CT
        self.CPW = CT // self.NWC
        self.NWP = 4 // self.NWC
        self.NTILE = CT * KT
        self.NREC = self.NTILE * 9 + KT


def swz(j):
    return j ^ ((j >> 1) & 4)


def loff(lane, dx, h):
    g, q, p = lane >> 4, (lane >> 2) & 3, lane & 3
    return swz(8 * g + q + 4 * h + dx) * 32 + p * 8


def kt_for(CT, Kmem):
    need = (Kmem + 15) // 16
    kt = 1 if need <= 1 else (2 if need <= 2 else 4)
    if CT == 3 and kt > 2:
        kt = 2
    return kt


def test_constants_match_kernel_source():
    src = open(os.path.join(os.path.dirname(__file__), "..", "mine_amd",
                            "ops", "csrc", "wrw_kernels.hip")).read()
    assert re.search(r"constexpr int R = 2;", src)
    assert re.search(r"constexpr int TW_ALL = 384;", src)
    assert re.search(r"XS = \(TW \+ 9\) \* 32;", src)
    assert re.search(r"GS = \(TW \+ 1\) \* 32;", src)
    assert re.search(r"return j \^ \(\(j >> 1\) & 4\);", src)
    assert re.search(
        r"swz\(8 \* g \+ q \+ 4 \* h \+ dx\) \* 32 \+ p \* 8;", src)
    assert re.search(r"NWC = CT == 3 \? 1 : CT;", src)


@pytest.mark.parametrize("CT,KT", CONFIGS)
def test_store_map_is_a_bijection(CT, KT):
    """Every (pixel, 16-byte half) of a sub-image row gets its own 16
    bytes, inside the sub-image's stride, for x (TW + 2 positions) and
    for gy (TW pixels)."""
    c = Cfg(CT, KT)
    for npix, stride in ((c.TW + 2, c.XS), (c.TW, c.GS)):
        offs = [swz(j) * 32 + half * 16
                for j in range(npix) for half in range(2)]
        assert len(set(offs)) == len(offs)
        assert min(offs) == 0 and max(offs) + 16 <= stride
        assert all(o % 16 == 0 for o in offs)
    assert c.STAGE_BYTES <= 80 * 1024


def _tr_read(mem, addr):
    """ds_read_b64_tr_b16 of one wave: mem is the LDS as 16-bit cells,
    addr[lane] in bytes. Returns out[lane][0..3]."""
    out = [[None] * 4 for _ in range(64)]
    for lane in range(64):
        g, i = lane >> 4, lane & 15
        for q in range(4):
            src_lane = 16 * g + 4 * q + (i >> 2)
            out[lane][q] = mem[addr[src_lane] // 2 + (i & 3)]
    return out


@pytest.mark.parametrize("dx", [0, 1, 2])
def test_transpose_reads_rebuild_the_mfma_operand(dx):
    npix = 96 + 8
    mem = [None] * (npix * 16)
    for j in range(npix):          # the staging store: pixel j, 2 halves
        for ch in range(16):
            mem[(swz(j) * 32) // 2 + ch] = (j, ch)
    for j0 in (0, 32, 64):         # chunk bases
        lo = _tr_read(mem, [j0 * 32 + loff(l, dx, 0) for l in range(64)])
        hi = _tr_read(mem, [j0 * 32 + loff(l, dx, 1) for l in range(64)])
        for lane in range(64):
            for e in range(8):
                got = (lo[lane] + hi[lane])[e]
                assert got == (j0 + 8 * (lane >> 4) + e + dx, lane & 15)


def _half_conflicts(addrs):
    """Pairs of lanes of one 32-lane half on one bank at different
    addresses; each 8-byte access covers two banks."""
    n = 0
    for half in (addrs[:32], addrs[32:]):
        for a in range(32):
            for b in range(a + 1, 32):
                if half[a] == half[b]:
                    continue
                ba = {(half[a] // 4 + d) % 64 for d in range(2)}
                bb = {(half[b] // 4 + d) % 64 for d in range(2)}
                n += bool(ba & bb)
    return n


@pytest.mark.parametrize("CT,KT", CONFIGS)
def test_transpose_reads_are_bank_conflict_free(CT, KT):
    c = Cfg(CT, KT)
    bases = []
    for slot in range(XSLOTS):                      # x ring
        for ct in range(CT):
            bases.append(slot * c.XROW + ct * c.XS)
    for r in range(R):                              # gy rows (dx = 0 only)
        for kt in range(KT):
            bases.append(c.X_BYTES + r * c.GROW + kt * c.GS)
    n_x = XSLOTS * CT
    for bi, base in enumerate(bases):
        for ch in range(c.TW // 32):
            for dx in ((0, 1, 2) if bi < n_x else (0,)):
                for h in range(2):
                    addrs = [base + ch * 1024 + loff(l, dx, h)
                             for l in range(64)]
                    assert all(a % 8 == 0 for a in addrs)
                    assert _half_conflicts(addrs) == 0


def test_plain_rows_would_conflict():
    """The check is not vacuous: plain 32-byte pixel rows without the
    half swap put the two 16-lane groups of a half on the same banks."""
    addrs = []
    for lane in range(64):
        g, q, p = lane >> 4, (lane >> 2) & 3, lane & 3
        addrs.append((8 * g + q) * 32 + p * 8)
    assert _half_conflicts(addrs) > 0


# ---------------------------------------------------------------------------
# the whole walk, in float64


def _reflect(v, n):
    if v < 0:
        v = -v
    if v >= n:
        v = 2 * (n - 1) - v
    return v


def _steps(r_begin, r_end, H):
    """The kernel's next_step(): (n, y0, ngr, py0, nxr) per step."""
    g, cont = r_begin, False
    while g < r_end:
        n, y = divmod(g, H)
        if not cont:
            cont = True
            yield (n, y, 0, y, 2)
        else:
            nr = min(R, H - y, r_end - g)
            g += nr
            if y + nr == H:
                cont = False
            yield (n, y, nr, y + 2, nr)


def _wrw_replay(x, gy, n_slabs):
    """x (N,H,W,C), gy (N,H,W,K) float64 -> dw (K,C,3,3), db (K) the way
    the two kernels compute them."""
    N, H, W, C = x.shape
    K = gy.shape[-1]
    Kmem = K if (K == 4 or K % 8 == 0) else (K + 7) // 8 * 8
    if Kmem != K:
        gy = F.pad(gy, (0, Kmem - K))
    CT = C // 16
    KT = kt_for(CT, Kmem)
    c = Cfg(CT, KT)
    k4 = Kmem == 4
    nkb = ((Kmem + 15) // 16 + KT - 1) // KT
    rows_total = N * H
    ws = torch.full((n_slabs, nkb, c.NREC, 64, 4), float("nan"),
                    dtype=torch.float64)
    lane = torch.arange(64)
    for slab in range(n_slabs):
        r_begin = rows_total * slab // n_slabs
        r_end = rows_total * (slab + 1) // n_slabs
        for kb in range(nkb):
            kb0 = kb * KT * 16
            # images as [sub-image][pixel slot][16 ch]; never-staged
            # cells stay zero like the kernel's initial fill
            xs = torch.zeros(XSLOTS, CT, c.TW + 9, 16, dtype=torch.float64)
            gs = torch.zeros(R, KT, c.TW + 1, 16, dtype=torch.float64)
            # per wave: acc[cp][kt][tap] as (16 k, 16 c), accb[kt] (16 k)
            acc = torch.zeros(4, c.CPW, KT, 9, 16, 16, dtype=torch.float64)
            accb = torch.zeros(4, KT, 16, dtype=torch.float64)
            for x0 in range(0, W, c.TW):
                Wt = min(W - x0, c.TW)
                nch = (Wt + 31) >> 5
                gpmax, jmax = nch * 32, nch * 32 + 1
                for (n, y0, ngr, py0, nxr) in _steps(r_begin, r_end, H):
                    for r in range(nxr):              # stage x
                        yy = _reflect(py0 + r - 1, H)
                        slot = (py0 + r) & (XSLOTS - 1)
                        for j in range(jmax + 1):
                            u = _reflect(x0 + j - 1, W)
                            u = min(max(u, 0), W - 1)
                            xs[slot, :, swz(j)] = x[n, yy, u].view(CT, 16)
                    for r in range(ngr):              # stage gy
                        for pp in range(gpmax):
                            v = torch.zeros(KT * 16, dtype=torch.float64)
                            if pp < Wt:
                                row = gy[n, y0 + r, x0 + pp]
                                if k4:
                                    v[:4] = row
                                else:
                                    m = min(KT * 16, Kmem - kb0)
                                    v[:m] = row[kb0:kb0 + m]
                            gs[r, :, swz(pp)] = v.view(KT, 16)
                    for wave in range(4):             # contract
                        cw, wp = wave % c.NWC, wave // c.NWC
                        for u in range(wp, ngr * nch, c.NWP):
                            row = 1 if u >= nch else 0
                            ch = u - row * nch
                            pix = ch * 32 + torch.arange(32)
                            a = gs[row][:, [swz(int(p)) for p in pix]]
                            if cw == 0:
                                accb[wave] += a.sum(1)
                            for dy in range(3):
                                slot = (y0 + row + dy) & (XSLOTS - 1)
                                for cp in range(c.CPW):
                                    ct = cw + cp * c.NWC
                                    for dx in range(3):
                                        b = xs[slot, ct][
                                            [swz(int(p) + dx) for p in pix]]
                                        for kt in range(KT):
                                            acc[wave, cp, kt, dy * 3 + dx] \
                                                += a[kt].T @ b
            # partial out: waves sharing tiles add up in wave order
            for wave in range(4):
                cw, wp = wave % c.NWC, wave // c.NWC

                def flush(rec, tile16):
                    # lane holds rows (lane>>4)*4 + r, column lane & 15
                    v = tile16[(lane >> 4)[:, None] * 4
                               + torch.arange(4)[None], (lane & 15)[:, None]]
                    if wp == 0:
                        ws[slab, kb, rec] = v
                    else:
                        ws[slab, kb, rec] += v

                for cp in range(c.CPW):
                    for kt in range(KT):
                        for t in range(9):
                            flush(((cw + cp * c.NWC) * KT + kt) * 9 + t,
                                  acc[wave, cp, kt, t])
                if cw == 0:
                    for kt in range(KT):
                        flush(c.NTILE * 9 + kt,
                              accb[wave, kt][:, None].expand(16, 16))
    # finishing kernel
    dw = torch.full((K, C, 3, 3), float("nan"), dtype=torch.float64)
    db = torch.full((K,), float("nan"), dtype=torch.float64)
    tot = ws.sum(0)
    for kb in range(nkb):
        for rec in range(c.NREC):
            for ln in range(64):
                for r in range(4):
                    if rec < c.NTILE * 9:
                        tile, tap = divmod(rec, 9)
                        ct, kt = divmod(tile, KT)
                        k = (kb * KT + kt) * 16 + (ln >> 4) * 4 + r
                        cc = ct * 16 + (ln & 15)
                        if k < K:
                            dw[k, cc, tap // 3, tap % 3] = tot[kb, rec, ln, r]
                    elif (ln & 15) == 0:
                        kt = rec - c.NTILE * 9
                        k = (kb * KT + kt) * 16 + (ln >> 4) * 4 + r
                        if k < K:
                            db[k] = tot[kb, rec, ln, r]
    return dw, db


# (32, 24): two c-groups x two pixel halves, two k tiles with a padded
# one, a partial last chunk; 3 slabs over 2 x 5 rows put one slab
# boundary inside image 0 and carry slab 1 across the image boundary.
# (16, 4): the 8-byte path, pixel split over four waves, two column
# tiles. (48, 40): three c-groups per wave, two k blocks on the grid.
@pytest.mark.parametrize("C,K,B,H,W,slabs", [(32, 24, 2, 5, 70, 3),
                                             (16, 4, 1, 3, 400, 2),
                                             (48, 40, 1, 4, 33, 2)])
def test_walk_matches_autograd(C, K, B, H, W, slabs):
    g = torch.Generator().manual_seed(C + K)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    gy = torch.randn(B, K, H, W, generator=g, dtype=torch.float64)
    w = torch.zeros(K, C, 3, 3, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w)
    (ref,) = torch.autograd.grad(y, w, gy)
    dw, db = _wrw_replay(x.permute(0, 2, 3, 1).contiguous(),
                         gy.permute(0, 2, 3, 1).contiguous(), slabs)
    torch.testing.assert_close(dw, ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(db, gy.sum((0, 2, 3)), rtol=1e-4, atol=1e-4)
