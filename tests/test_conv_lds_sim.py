"""CPU replay of conv3x3_fwd_kernel's LDS image (ops/csrc/conv_kernels.hip).

No GPU needed. Three things are replayed from the kernel's own index
arithmetic:
  * the B-fragment ds_read_b128 addresses of every (chunk, row) against
    the gfx950 bank map — bank = (byte address / 4) mod 64, served in
    four fixed groups of 16 lanes — asserting zero conflicting pairs;
  * the division-free staging walk (StageIdx), asserting that it writes
    every (cb, row, x) vector of the image exactly once;
  * the whole tile: staged image + packed weights + swapped-operand lane
    map against F.conv2d, for the reflect forward.
"""
import os
import re

import pytest
import torch
import torch.nn.functional as F

K_BLOCK = 256
TILE_W, TILE_H = 64, 4
STAGE_W, STAGE_H = TILE_W + 2, TILE_H + 2
ROW_PITCH = STAGE_W                      # 16-byte vectors
CB_PITCH = STAGE_H * ROW_PITCH + 10

# ds_read_b128 lane groups on gfx950, one LDS cycle each when conflict-free
LANE_GROUPS = [
    [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
    [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31],
    [32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59],
    [36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63],
]


def seg_vec_off(seg, nseg):
    s = seg if seg < nseg else nseg - 1
    cb, tap = divmod(s, 9)
    return cb * CB_PITCH + (tap // 3) * ROW_PITCH + (tap % 3)


def read_vec(cv, kc, row, wave, lane):
    """16-byte vector index the lane reads for chunk kc of output row."""
    p, g = lane & 15, lane >> 4
    return seg_vec_off(kc * 4 + g, 9 * cv) + row * ROW_PITCH + wave * 16 + p


def test_constants_match_kernel_source():
    src = open(os.path.join(os.path.dirname(__file__), "..", "mine_amd",
                            "ops", "csrc", "conv_kernels.hip")).read()
    assert re.search(r"TILE_W = 64;", src)
    assert re.search(r"TILE_H = 4;", src)
    assert re.search(r"ROW_PITCH = STAGE_W;", src)
    assert re.search(r"CB_PITCH = STAGE_H \* ROW_PITCH \+ 10;", src)


@pytest.mark.parametrize("C", [8, 16, 32, 48, 64])
def test_b_fragment_reads_are_bank_conflict_free(C):
    cv = C // 8
    nch = (9 * cv + 3) // 4
    conflicts = 0
    for kc in range(nch):          # every (tap, cb) the kernel reads ...
        for row in range(TILE_H):  # ... under every output row
            for wave in range(4):
                for grp in LANE_GROUPS:
                    addr = [16 * read_vec(cv, kc, row, wave, l) for l in grp]
                    for i in range(16):
                        for j in range(i + 1, 16):
                            if addr[i] == addr[j]:
                                continue  # same address: broadcast
                            bi = {(addr[i] // 4 + d) % 64 for d in range(4)}
                            bj = {(addr[j] // 4 + d) % 64 for d in range(4)}
                            conflicts += bool(bi & bj)
    assert conflicts == 0


def test_unpadded_image_would_conflict():
    """The check above is not vacuous: the previous image (pixel-major,
    C bf16 per pixel, no padding) conflicts at C=64."""
    cv = 8
    grp = LANE_GROUPS[0]
    addr = []
    for l in grp:
        p, g = l & 15, l >> 4
        cb, tap = divmod(g, 9)
        addr.append((((tap // 3) * STAGE_W + p + tap % 3) * cv + cb) * 16)
    banks = [(a // 4) % 64 for a in addr]
    assert len(set(banks)) < len(set(addr))


class StageIdx:
    """Mirror of the kernel's StageIdx<CV>."""

    def __init__(self, cv_n, tid):
        self.n = cv_n
        self.px_step = K_BLOCK // cv_n
        self.cv_step = K_BLOCK % cv_n
        self.cv = tid % cv_n
        self.x = tid // cv_n
        self.row = 0
        for _ in range(3):
            if self.x >= STAGE_W:
                self.x -= STAGE_W
                self.row += 1

    def next(self):
        self.x += self.px_step % STAGE_W
        self.row += self.px_step // STAGE_W
        if self.cv_step:
            self.cv += self.cv_step
            if self.cv >= self.n:
                self.cv -= self.n
                self.x += 1
        if self.x >= STAGE_W:
            self.x -= STAGE_W
            self.row += 1


def staged_slots(cv_n):
    nit = (STAGE_H * STAGE_W * cv_n + K_BLOCK - 1) // K_BLOCK
    out = []
    for tid in range(K_BLOCK):
        si = StageIdx(cv_n, tid)
        for _ in range(nit):
            if si.row < STAGE_H:
                assert 0 <= si.x < STAGE_W and 0 <= si.cv < cv_n
                out.append((si.cv, si.row, si.x))
            si.next()
    return out


@pytest.mark.parametrize("cv_n", [1, 2, 3, 4, 5, 6, 7, 8])
def test_staging_walk_covers_image_once(cv_n):
    slots = staged_slots(cv_n)
    assert len(slots) == len(set(slots)) == cv_n * STAGE_H * STAGE_W
    top = max(cv * CB_PITCH + r * ROW_PITCH + x for cv, r, x in slots)
    assert top < cv_n * CB_PITCH          # inside the LDS allocation
    # and the furthest read stays inside it too
    nch = (9 * cv_n + 3) // 4
    far = max(read_vec(cv_n, kc, TILE_H - 1, 3, l)
              for kc in range(nch) for l in range(64))
    assert far < cv_n * CB_PITCH


def reflect(v, n):
    if v < 0:
        v = -v
    if v >= n:
        v = 2 * (n - 1) - v
    return min(max(v, 0), n - 1)


@pytest.mark.parametrize("C,K", [(16, 4), (24, 24)])
def test_tile_math_matches_conv2d(C, K):
    """One workgroup's tile, lane by lane, in integer-valued fp32."""
    from mine_amd.ops.conv import _pack_lut
    cv_n = C // 8
    H, W = 6, 70
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-3, 4, (C, H, W), generator=g).float()
    w = torch.randint(-2, 3, (K, C, 3, 3), generator=g).float()
    ref = F.conv2d(F.pad(x[None], (1, 1, 1, 1), mode="reflect"), w)[0]
    lut = _pack_lut(K, C, False, torch.device("cpu"))
    wp = torch.cat((w.reshape(-1), w.new_zeros(1)))[lut].view(-1, 8)
    nseg = 9 * cv_n
    nch = (nseg + 3) // 4
    nk = (K + 15) // 16
    x_nhwc = x.permute(1, 2, 0)
    for x0, y0 in [(0, 0), (64, 4)]:
        lds = torch.full((cv_n * CB_PITCH, 8), float("nan"))
        for cv, r, sx in staged_slots(cv_n):
            yy = reflect(y0 + r - 1, H)
            xx = reflect(x0 + sx - 1, W)
            lds[cv * CB_PITCH + r * ROW_PITCH + sx] = \
                x_nhwc[yy, xx, cv * 8:cv * 8 + 8]
        for wave in range(4):
            if x0 + wave * 16 >= W:
                continue
            for r in range(TILE_H):
                if y0 + r >= H:
                    continue
                for a in range(nk):
                    # D[row = out channel][col = pixel]
                    d = torch.zeros(16, 16)
                    for kc in range(nch):
                        for lane_w in range(64):
                            gw, j = lane_w >> 4, lane_w & 15
                            wf = wp[(a * nch + kc) * 64 + lane_w]
                            for p in range(16):
                                lane = gw * 16 + p   # same k-group
                                b = lds[read_vec(cv_n, kc, r, wave, lane)]
                                if kc * 4 + gw >= nseg:
                                    b = torch.zeros(8)
                                d[j, p] += (wf * b).sum()
                    for lane in range(64):
                        p, gq = lane & 15, lane >> 4
                        pix = x0 + wave * 16 + p
                        if pix >= W:
                            continue
                        for c in range(4):
                            kout = a * 16 + gq * 4 + c
                            if kout < K:
                                assert d[gq * 4 + c, p] == \
                                    ref[kout, y0 + r, pix]
