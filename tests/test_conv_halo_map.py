"""CPU: the address map of the halo-resident conv A image (csrc/gemm_conv_halo.h),
walked exhaustively through hvit_conv_halo_off for every (W, Cin, tile rows) the
default model's 3x3 convs present to it.

* every (halo pixel, 16-byte channel chunk) has a slot of its own, inside the
  image, and a pixel's chunks stay inside the pixel's 2 Cin bytes (the DMA fills
  the image in lane-linear 1-KiB pieces: a slot's source chunk is found from the
  slot alone);
* every A fragment read of every tap is conflict-free by the LDS banking rule of
  ds_read_b128: bank (a / 4) mod 64, four dwords per lane, conflicts only inside
  each of the four 16-lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31},
  {32-35, 44-47, 52-59}, {36-43, 48-51, 60-63}.  A fragment is 16 consecutive
  output pixels (lane & 15) x four chunks (lane >> 4) of one 64-channel stage and
  k-step; W = 16 and W = 32 tiles, where a fragment covers a whole image row or
  half of one, are among the cases.

What this walks is halo_off(), which the kernel's DMA side uses through halo_key().
The kernel's read side forms the same address incrementally (fragment base + uniform
tap offset + the lane's swizzled chunk); that it equals halo_off() is shown by the
bitwise and NaN-halo checks of tests/test_gpu_conv_halo.py, not here.
"""

import pytest

# (H, W, Cin of the A operand, tile rows): forward enc1 / enc2, data gradients
# enc1, enc2 (fits beside a 64-column ring only), dec2, dec1, dec0; 128- and 256-row tiles
CASES = [
    (128, 128, 64, 128), (128, 128, 64, 256),
    (64, 64, 128, 128), (64, 64, 128, 256),
    (128, 128, 128, 128), (128, 128, 128, 256),
    (64, 64, 256, 128),
    (64, 64, 64, 128), (64, 64, 64, 256),
    (32, 32, 128, 128), (32, 32, 128, 256),
    (16, 16, 256, 128), (16, 16, 256, 256),
    (8, 256, 64, 128), (8, 256, 64, 256),  # W % rows == 0: a whole-row segment
]
GROUPS = [
    list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
    list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
    list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
    list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64)),
]


def tile_dims(W, rows):
    tw = min(W, rows)
    return tw, rows // tw


@pytest.fixture(scope="module")
def off(hv):
    f = hv._lib.lib().hvit_conv_halo_off
    return lambda *a: f(*a)


@pytest.mark.parametrize("case", CASES)
def test_halo_slots_distinct(off, case):
    H, W, C, rows = case
    tw, tr = tile_dims(W, rows)
    seen = set()
    for hy in range(tr + 2):
        for hx in range(tw + 2):
            base = (hy * (tw + 2) + hx) * 2 * C
            for cc in range(C // 8):
                a = off(H, W, C, rows, hy, hx, cc)
                assert a >= 0 and a % 16 == 0
                assert base <= a < base + 2 * C, (hy, hx, cc, a)
                # the swizzle permutes inside the chunk's group of eight (sixteen from 256-byte pixels on)
                grp = 8 if C == 64 else 16
                assert (a - base) // (16 * grp) == cc // grp
                seen.add(a)
    assert len(seen) == (tr + 2) * (tw + 2) * (C // 8)
    assert max(seen) + 16 == (tr + 2) * (tw + 2) * 2 * C


@pytest.mark.parametrize("case", CASES)
def test_halo_fragment_reads_conflict_free(off, case):
    H, W, C, rows = case
    tw, tr = tile_dims(W, rows)
    for rb in range(0, rows, 16):        # fragment: tile rows rb .. rb + 15
        for ky in range(3):
            for kx in range(3):
                for c0 in range(0, C, 64):
                    for s in range(2):
                        addr = []
                        for lane in range(64):
                            r = rb + (lane & 15)
                            ty, tx = divmod(r, tw)
                            addr.append(off(H, W, C, rows, ty + ky, tx + kx, c0 // 8 + 4 * s + (lane >> 4)))
                        for grp in GROUPS:
                            banks = {}
                            for lane in grp:
                                for d in range(4):
                                    b = (addr[lane] // 4 + d) % 64
                                    assert banks.setdefault(b, addr[lane]) == addr[lane], \
                                        f"bank conflict: rows {rb}.., tap ({ky},{kx}), c0 {c0}, k-step {s}"


def test_halo_geometry_refusals(off):
    # neither whole rows nor a row segment; a tile that would span images; thin or odd channel counts
    assert off(96, 96, 64, 128, 0, 0, 0) == -1
    assert off(40, 24, 64, 128, 0, 0, 0) == -1
    assert off(8, 8, 64, 128, 0, 0, 0) == -1
    assert off(16, 16, 256, 128, 0, 0, 0) == 0
    assert off(24, 16, 64, 256, 0, 0, 0) == -1   # 24 rows of 16: 256-row tiles would span images
    assert off(128, 128, 32, 128, 0, 0, 0) == -1
    assert off(128, 128, 192, 128, 0, 0, 0) == -1
    assert off(128, 128, 64, 64, 0, 0, 0) == -1
