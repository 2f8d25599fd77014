"""K1x's output layer on the B operand's lane-group broadcast, emulated on the CPU: the register image that `l4_k` / `l4_dim` / `l4_bias_dim`
(psnode_mfma_x.h, mirrored here) describe, fed through a numpy model of the 16-block v_mfma_f32_4x4x1 with BLGP 1 / 2, the merge of the two
chains, the v_permlane16_swap fold and the two DPP row rotations, must give W4 @ act + b4 in the state layout (row rho of 16 lanes holds dims
4 (rho >> 1) + 2 (rho & 1) and the next one, for trajectory lane & 3, in every block of the row)."""
import numpy as np
import pytest

LANES = np.arange(64)


# ---- mirrors of psnode_mfma_x.h
def l4_k(m, lane):
    return 32 * (m >> 2) + 4 * ((lane >> 2) & 7) + (m & 3)


def l4_dim(lane):
    return 4 * (lane >> 5) + (lane & 3)


def l4_bias_dim(r, lane):
    return 4 * (lane >> 5) + r if ((lane >> 2) & 7) == 0 else -1


def pack_image(W4, b4, xd, H):
    """pack_x_kernel's W4A / B4C branches: 8 A registers and the 4 C registers of the lo chain, [reg][lane]."""
    a = np.zeros((8, 64), np.float32)
    c = np.zeros((4, 64), np.float32)
    for lane in range(64):
        for m in range(8):
            d, k = l4_dim(lane), l4_k(m, lane)
            if d < xd and k < H:
                a[m, lane] = W4[d, k]
        for r in range(4):
            d = l4_bias_dim(r, lane)
            if 0 <= d < xd:
                c[r, lane] = b4[d]
    return a, c


# ---- the instructions
def mfma_4x4x1(a, b, c, blgp):
    """D_blk[r][col] = C_blk[r][col] + A_blk[r] * B_blk'[col]: A / B one value per lane (block, index), C / D register r of lane (block, col).
    BLGP 1: every block reads B from lanes 0..31 (lane & 31), 2: from lanes 32..63."""
    src = {0: LANES, 1: LANES & 31, 2: 32 + (LANES & 31)}[blgp]
    bsel = b[src]
    d = np.empty((4, 64), np.float32)
    for r in range(4):
        d[r] = c[r] + a[(LANES & ~3) + r] * bsel
    return d


def permlane16_swap(a, b):
    """Odd rows of the first register <-> even rows of the second."""
    a2, b2 = a.copy(), b.copy()
    for row in (0, 2):
        lo, hi = slice(16 * row, 16 * row + 16), slice(16 * row + 16, 16 * row + 32)
        a2[hi], b2[lo] = b[lo], a[hi]
    return a2, b2


def row_ror_add(x, n):
    return (x + x[(LANES & ~15) + ((LANES & 15) + n) % 16]).astype(np.float32)


def l4_out(a, c, hA):
    lo, hi = c.copy(), np.zeros((4, 64), np.float32)
    for cc in range(4):
        lo = mfma_4x4x1(a[cc], hA[cc], lo, 1)
        hi = mfma_4x4x1(a[4 + cc], hA[cc], hi, 2)
    q = lo + hi
    e0, e1 = permlane16_swap(q[0], q[2])
    o0, o1 = permlane16_swap(q[1], q[3])
    k = [e0 + e1, o0 + o1]
    return [row_ror_add(row_ror_add(v, 8), 4) for v in k]


@pytest.mark.parametrize("xd,H", [(8, 64), (8, 33), (8, 32), (5, 20), (4, 64), (1, 1), (7, 63)])
def test_image_and_fold_reproduce_the_output_layer(xd, H):
    rng = np.random.default_rng(100 * xd + H)
    W4 = rng.uniform(-1, 1, (xd, H)).astype(np.float32)
    b4 = rng.uniform(-1, 1, xd).astype(np.float32)
    act = np.zeros((64, 4), np.float32)
    act[:H] = rng.uniform(-1, 1, (H, 4))
    a, c = pack_image(W4, b4, xd, H)
    hA = np.stack([act[4 * (LANES >> 2) + cc, LANES & 3] for cc in range(4)])          # A layout: lane (b, t) register cc = act[4b + cc][t]
    k = l4_out(a, c, hA)
    want = W4.astype(np.float64) @ act[:H].astype(np.float64) + b4[:, None]
    for lane in range(64):
        rho, t = lane >> 4, lane & 3
        for e in range(2):
            d = 4 * (rho >> 1) + 2 * (rho & 1) + e
            ref = want[d, t] if d < xd else 0.0
            assert abs(k[e][lane] - ref) <= 1e-5 * max(1.0, abs(ref)), (lane, e, d, float(k[e][lane]), ref)


def test_every_weight_and_bias_sits_in_exactly_one_lane_of_the_image():
    seen = np.zeros((8, 64), int)
    for lane in range(64):
        for m in range(8):
            seen[l4_dim(lane), l4_k(m, lane)] += 1
    assert (seen == 1).all()
    bias = np.zeros(8, int)
    for lane in range(64):
        for r in range(4):
            if l4_bias_dim(r, lane) >= 0:
                bias[l4_bias_dim(r, lane)] += 1
    assert (bias == 4).all()          # one block per dim-tile, its four columns (trajectories)
