"""The preview denoiser (include/rtw_denoise.h) restated in numpy: whole-image f32 arrays, 9 shifted arrays for
the prep pass and 25 per level, sequential f32 adds in the header's order.  Every intermediate is float32;
`denoise` gives the bits of rtw_denoise_host and of the device kernels."""
import numpy as np

f32 = np.float32
H5 = [f32(1 / 16), f32(1 / 4), f32(3 / 8), f32(1 / 4), f32(1 / 16)]
K3 = [f32(1 / 4), f32(1 / 2), f32(1 / 4)]
INF = f32(np.inf)
NAN = f32(np.nan)


def finite(a):
    return np.abs(a) < INF


def shift(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` where that lies outside the image."""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    if abs(dy) >= H or abs(dx) >= W:
        return b
    b[max(0, -dy):min(H, H - dy), max(0, -dx):min(W, W - dx)] = a[max(0, dy):min(H, H + dy), max(0, dx):min(W, W + dx)]
    return b


def prep(color, se, guide):
    """(H, W, 4) records {r, g, b, g_p}."""
    l = (color[..., 0] + color[..., 1]) + color[..., 2]
    v = se * se
    vl = (v[..., 0] + v[..., 1]) + v[..., 2]
    ok = finite(l) & finite(vl)
    if guide is not None:
        for c in range(guide.shape[-1]):
            ok = ok & finite(guide[..., c])
    m = np.where(ok, vl, NAN)
    sk = np.zeros(m.shape, f32)
    sv = np.zeros(m.shape, f32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            kk = K3[dy + 1] * K3[dx + 1]
            q = shift(m, dy, dx, NAN)
            okq = finite(q)
            sk = np.where(okq, sk + kk, sk)
            sv = np.where(okq, sv + kk * q, sv)
    g = np.where(ok, sv / sk, NAN)
    R = np.concatenate([color, g[..., None]], axis=-1)
    assert R.dtype == np.float32 and sk.dtype == np.float32 and sv.dtype == np.float32
    return R


def level(R, G, step, sigma_l, inv_sg2):
    w_p = R[..., 3]
    ok = finite(w_p)
    lp = (R[..., 0] + R[..., 1]) + R[..., 2]
    sw = np.zeros(w_p.shape, f32)
    sc = [np.zeros(w_p.shape, f32) for _ in range(3)]
    s2 = np.zeros(w_p.shape, f32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            Q = shift(R, dy * step, dx * step, NAN)  # (outside: w = NaN, skipped)
            take = finite(Q[..., 3])
            lq = (Q[..., 0] + Q[..., 1]) + Q[..., 2]
            x = np.abs(lq - lp) / (sigma_l * np.sqrt(w_p + Q[..., 3]) + f32(1e-6))
            wl = f32(1) / (f32(1) + x * x)
            if G is not None:
                Gq = shift(G, dy * step, dx * step, f32(0))
                d2 = np.zeros(w_p.shape, f32)
                for c in range(G.shape[-1]):
                    d = Gq[..., c] - G[..., c]
                    d2 = d2 + d * d
                t = f32(1) - d2 * inv_sg2
                t = np.where(t < 0, f32(0), t)
                wg = t * t
            else:
                wg = f32(1)
            w = (H5[dy + 2] * H5[dx + 2]) * (wl * wg)
            assert w.dtype == np.float32
            sw = np.where(take, sw + w, sw)
            for c in range(3):
                sc[c] = np.where(take, sc[c] + w * Q[..., c], sc[c])
            s2 = np.where(take, s2 + (w * w) * Q[..., 3], s2)
    out = np.stack([sc[0] / sw, sc[1] / sw, sc[2] / sw, s2 / (sw * sw)], axis=-1)
    out = np.where(ok[..., None], out, R)
    assert out.dtype == np.float32
    return out


def denoise(color, se, guide, size, iterations=3, sigma_l=1.5, sigma_g=0.35):
    """color, se: (W*H, 3) f32; guide: (W*H, gc) f32 or None; size = (W, H).  Returns ((W*H, 3), (W*H,))."""
    W, H = size
    color = np.asarray(color).reshape(H, W, 3)
    se = np.asarray(se).reshape(H, W, 3)
    assert color.dtype == np.float32 and se.dtype == np.float32
    if guide is not None:
        guide = np.asarray(guide)
        assert guide.dtype == np.float32
        guide = guide.reshape(H, W, -1) if guide.size else None
    sigma_l, sigma_g = f32(sigma_l), f32(sigma_g)
    with np.errstate(all="ignore"):
        inv_sg2 = f32(1) / (sigma_g * sigma_g)
        R = prep(color, se, guide)
        for i in range(iterations):
            R = level(R, guide, 1 << i, sigma_l, inv_sg2)
    assert R.dtype == np.float32
    return np.ascontiguousarray(R[..., :3]).reshape(-1, 3), np.ascontiguousarray(R[..., 3]).reshape(-1)


def synthetic(size, gc, seed):
    """Seeded inputs of the synthetic cases: ordinary pixels (a smooth ramp plus noise, the standard error
    matching the noise) mixed with NaN and +-inf colours, NaN, inf and zero standard errors, a NaN guide channel,
    values near 1e30 and negative colours.  Returns (color, se, guide or None), shaped (W*H, ...)."""
    W, H = size
    n = W * H
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (f32(0.2) + f32(0.6) * (xx + 2 * yy).astype(f32) / f32(W + 2 * H)).reshape(n, 1)
    se = (f32(0.02) + f32(0.2) * rng.random((n, 3), dtype=f32)).astype(f32)
    color = (base * (f32(0.5) + rng.random((1, 3), dtype=f32)) + se * rng.standard_normal((n, 3)).astype(f32)).astype(f32)
    guide = None
    if gc:
        guide = (rng.random((n, gc), dtype=f32) * f32(0.3) + (xx.reshape(n, 1) > W // 2).astype(f32)).astype(f32)
    special = rng.permutation(n)
    k = max(1, n // 24)  # about half of the pixels stay ordinary

    def pick(j):  # the pixels of special kind j (small frames: kinds 0, 5 and 10 only, one pixel each)
        if n >= 24:
            return special[j::12][:k]
        return special[j // 5:j // 5 + 1] if j % 5 == 0 else special[:0]

    color[pick(0), 0] = np.nan
    color[pick(1), 1] = np.inf
    color[pick(2), 2] = -np.inf
    se[pick(3), 0] = np.nan
    se[pick(4), 1] = np.inf
    se[pick(5)] = 0
    if gc:
        guide[pick(6), gc - 1] = np.nan
    color[pick(7)] = f32(1e30) * (f32(0.5) + rng.random((len(pick(7)), 3), dtype=f32))
    se[pick(8), 2] = f32(1e30)  # squares to inf: left out
    se[pick(9)] = f32(3e14)  # squares to about 1e29: kept
    color[pick(10)] = -color[pick(10)]
    return color, se, guide


# ---- the synthetic cases shared by test_denoise_host.py and test_gpu_denoise.py ----------------------
SIZES = [(2, 2), (5, 3), (37, 23), (64, 4), (65, 5), (130, 9)]
CHANNELS = [0, 1, 3, 4]


def cases():
    """(size, guide channels, iterations, seed): every size with every channel count, the iterations 1..6 spread
    over them so that every size meets steps of 16 and 32 (beyond the image) and every count of iterations."""
    out = []
    for i, size in enumerate(SIZES):
        for j, gc in enumerate(CHANNELS):
            out.append((size, gc, 1 + (i + 2 * j + (3 if gc == 0 else 0)) % 6, 100 * i + j))
        out.append((size, 3, 6, 100 * i + 50))
        out.append((size, 0, 5, 100 * i + 51))
    return out


CASES = cases()
assert {c[2] for c in CASES} == {1, 2, 3, 4, 5, 6}


def case_id(c):
    return f"{c[0][0]}x{c[0][1]}-gc{c[1]}-it{c[2]}"
