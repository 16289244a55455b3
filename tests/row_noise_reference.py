"""The per-row keyed sampling noise (lfi_row_noise, csrc/lfi_noise.hip) restated in numpy: integer Philox4x32-10 and
fp64 Box-Muller, plus the per-element error bound the GPU tests hold the fp32 kernel to. No device, no library.

For a row with 64-bit key K taking the frame at 64-bit position p, candidate k, channel c:
    o[0..3] = philox4x32_10(counter (c >> 2, lo32(p), hi32(p), k), key (lo32(K), hi32(K)))
    u_j = (o_j >> 9) * 2^-23 + 2^-24
    g0 = sqrt(-2 ln u0) cos(2 pi u1), g1 = sqrt(-2 ln u0) sin(2 pi u1); g2, g3 likewise from (u2, u3)
    channel c takes g[c & 3]; z = eps * g
The `defect` argument plants one of four mistakes (tests/test_row_noise_cpu.py checks that each moves the output)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
G_MAX = float(np.sqrt(48.0 * np.log(2.0)))      # |g| <= sqrt(-2 ln 2^-24)
DEFECTS = ("nine_rounds", "swapped_key_words", "dropped_hi_pos", "candidate_in_wrong_word")


def philox4x32(counter, key, rounds=10):
    """counter: four uint32 arrays (broadcastable), key: two -> four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.asarray(v, dtype=np.uint64) & MASK for v in key)
    for _ in range(rounds):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]       # 32 x 32 -> 64 bits: no overflow in uint64
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [h1 ^ c[1] ^ k0, l1, h0 ^ c[3] ^ k1, l0]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return [v.astype(np.uint32) for v in c]


def _words(keys, pos, n, ncand, C, defect=None):
    """The Philox outputs of every (frame i, row r, candidate k, quad q) -> four (n, B, K, Q) uint32 arrays, and (K, Q)."""
    assert defect is None or defect in DEFECTS, defect
    keys = np.array([int(v) & (2 ** 64 - 1) for v in np.atleast_1d(keys)], dtype=np.uint64)
    pos = np.array([int(v) & (2 ** 64 - 1) for v in np.atleast_1d(pos)], dtype=np.uint64)
    if pos.size == 1 and keys.size > 1:
        pos = np.repeat(pos, keys.size)
    assert keys.shape == pos.shape and keys.ndim == 1
    K, Q = max(int(ncand), 1), (C + 3) // 4
    with np.errstate(over="ignore"):
        p = pos[None, :] + np.arange(n, dtype=np.uint64)[:, None]           # (n, B), wraps mod 2^64 as the kernel's does
    p = p[:, :, None, None]
    key = keys[None, :, None, None]
    k = np.arange(K, dtype=np.uint64)[None, None, :, None]
    q = np.arange(Q, dtype=np.uint64)[None, None, None, :]
    k_lo, k_hi = key & MASK, key >> np.uint64(32)
    p_lo, p_hi = p & MASK, p >> np.uint64(32)
    if defect == "swapped_key_words":
        k_lo, k_hi = k_hi, k_lo
    if defect == "dropped_hi_pos":
        p_hi = np.zeros_like(p_hi)
    counter = (k, p_lo, p_hi, q) if defect == "candidate_in_wrong_word" else (q, p_lo, p_hi, k)
    o = philox4x32(counter, (k_lo, k_hi), rounds=9 if defect == "nine_rounds" else 10)
    return [np.broadcast_to(v, (n, keys.size, K, Q)) for v in o], K, Q


def _uniforms(o):
    return [(v >> np.uint32(9)).astype(np.float64) * 2.0 ** -23 + 2.0 ** -24 for v in o]


def _gather(g, n, B, K, Q, C):
    """Four (n, B, K, Q) arrays -> (n, B, K, C): channel c takes g[c & 3] of quad c >> 2."""
    return np.stack(g, axis=-1).reshape(n, B, K, 4 * Q)[..., :C]


def row_noise(keys, pos, n, ncand=0, eps=1.0, C=4, defect=None):
    """-> float64 (n, B, max(ncand, 1), C): eps_f32 * g for frames pos .. pos + n - 1 of every row, every candidate and channel. eps
    is rounded to fp32 first, as the kernel receives it."""
    o, K, Q = _words(keys, pos, n, ncand, C, defect)
    u = _uniforms(o)
    g = []
    for a, b in ((u[0], u[1]), (u[2], u[3])):
        rad = np.sqrt(-2.0 * np.log(a))
        g += [rad * np.cos(2.0 * np.pi * b), rad * np.sin(2.0 * np.pi * b)]
    return float(np.float32(eps)) * _gather(g, n, o[0].shape[1], K, Q, C)


def _ulp32(x):
    """The fp32 spacing at |x| (fp64 in, fp64 out); the smallest normal's spacing below it."""
    a = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), float(np.finfo(np.float32).tiny)).astype(np.float32)
    return np.spacing(a).astype(np.float64)


def row_noise_bound(keys, pos, n, ncand=0, eps=1.0, C=4, libm_ulp=4.0):
    """The error model of the fp32 kernel, per element -> float64 (n, B, max(ncand, 1), C), |kernel - row_noise| is allowed 2 x this.
    u is exact in fp32. With L = logf(u0), x = -2 L (exact scaling), rad = sqrtf(x), t = cospif / sinpif of the EXACT angle 2 u1 (a
    power-of-two multiple of an exact fp32 value: the kernel's sincospif form has no angle rounding; a kernel that rounds 2 pi u1 to
    fp32 would add rad * (half an ulp of the angle + u1 * |fl(2 pi) - 2 pi|) here):
        |dL| <= libm_ulp ulp(L)           -> |dx| = 2 |dL|, which reaches rad as |dx| / (2 rad)
        |drad| <= libm_ulp ulp(rad) + |dx| / (2 rad)
        |dt| <= libm_ulp ulp(t)
        g = fl(rad * t): |t| |drad| + rad |dt| + ulp(g) / 2;   z = fl(eps * g): eps |dg| + ulp(z) / 2
    libm_ulp = 4 is a margin over the 1 - 2 ulp HIP documents for logf, sqrtf and sincospif."""
    o, K, Q = _words(keys, pos, n, ncand, C)
    u = _uniforms(o)
    e = float(np.float32(eps))
    out = []
    for a, b in ((u[0], u[1]), (u[2], u[3])):
        L = np.log(a)
        rad = np.sqrt(-2.0 * L)
        d_rad = libm_ulp * _ulp32(rad) + 2.0 * libm_ulp * _ulp32(L) / (2.0 * rad)
        for t in (np.cos(2.0 * np.pi * b), np.sin(2.0 * np.pi * b)):
            d_t = libm_ulp * _ulp32(t)
            d_g = np.abs(t) * d_rad + rad * d_t + 0.5 * _ulp32(rad * t)
            out.append(abs(e) * d_g + 0.5 * _ulp32(e * rad * t))
    return _gather(out, n, o[0].shape[1], K, Q, C)
