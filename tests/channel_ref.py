"""NumPy statement of the measurement channel's tick (include/abrk.h, abrk_channel_step_batch) - TEST AID ONLY: a
vectorised Philox4x32-10, the normal built from it, and ChannelRef, which steps B rows one tick per call in the
arithmetic type of the kernel under test.  Where the tick says fma NumPy has none: in fp64 the reference rounds twice
(product, then sum - the tests' tolerances say so), in fp32 it forms product and sum in fp64, where the product of two
fp32 values is exact, and rounds the sum to fp32."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32(counter, key):
    """counter: four broadcastable integer arrays (words 0..3), key: (k0, k1) -> the four output words, uint64 arrays
    holding 32-bit values"""
    c = [np.asarray(w, dtype=np.uint64) & _LO for w in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]  # 32 x 32 bits: no overflow of 64
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _LO]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def words(seed, row, tick, col):
    """the output words of (seed, global row, tick, column); row may be negative (64-bit two's complement)"""
    r = np.asarray(row, dtype=np.int64).astype(np.uint64)
    seed = int(seed)
    return philox4x32((r & _LO, r >> _S32, np.asarray(tick, dtype=np.int64).astype(np.uint64),
                       np.asarray(col, dtype=np.int64).astype(np.uint64)), (seed & 0xFFFFFFFF, seed >> 32))


def normal(seed, row, tick, col):
    """the standard normal n of the tick, fp64"""
    w = words(seed, row, tick, col)
    k1 = (w[0] >> np.uint64(5)).astype(np.float64) * 2.0 ** 26 + (w[1] >> np.uint64(6)).astype(np.float64)
    k2 = (w[2] >> np.uint64(5)).astype(np.float64) * 2.0 ** 26 + (w[3] >> np.uint64(6)).astype(np.float64)
    u1, u2 = (k1 + 1.0) * 2.0 ** -53, k2 * 2.0 ** -53
    return np.sqrt(-2.0 * np.log(u1)) * np.cos((2.0 * np.pi) * u2)


def normal_block(seed, rows, ticks, cols):
    """n[b, t, c] for the global rows `rows`, ticks `ticks`, columns `cols` (1-D arrays)"""
    rows, ticks, cols = (np.asarray(v, dtype=np.int64) for v in (rows, ticks, cols))
    return normal(seed, rows[:, None, None], ticks[None, :, None], cols[None, None, :])


def statistics(n):
    """n[b, t, c] of standard normals -> {name: deviation in standard errors}: the mean (se 1 / sqrt N), the variance
    (se sqrt(2 / N)), and the mean products of neighbours along ticks, rows and columns (se 1 / sqrt(pairs))"""
    z = {"mean": n.mean() * np.sqrt(n.size), "variance": (np.mean(n * n) - 1.0) / np.sqrt(2.0 / n.size)}
    for name, a, b in (("tick-to-tick", n[:, 1:], n[:, :-1]), ("row-to-row", n[1:], n[:-1]),
                       ("column-to-column", n[:, :, 1:], n[:, :, :-1])):
        z[name] = np.mean(a * b) * np.sqrt(a.size)
    return z


def _fma(a, b, c, T):
    if T == np.float32:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    return a * b + c


def lowpass_gain(dt, tau):
    return -np.expm1(-dt / tau) if tau > 0 else 1.0


class ChannelRef:
    """B rows of a channel of `width` columns; tick(x) -> (out, dy) with x [B, width] (the concatenated inputs); dy is
    None without `difference`.  `counter` may be zero-filled between ticks.  `v_hist` keeps every tick's v before the
    quantisation as v * inv_res (fp64 product of the T values), for the tests' distance-from-a-tie checks."""

    def __init__(self, width, B, bias=0.0, sigma=0.0, resolution=0.0, delay=0, difference=False, tau_diff=0.0, dt=0.001,
                 seed=0, row_offset=0, dtype=np.float64):
        T = self.T = np.dtype(dtype).type
        self.W, self.B, self.d, self.difference = width, B, int(delay), difference
        col = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (width,)).copy()
        self.bias, self.sigma, self.res = col(bias).astype(T), col(sigma).astype(T), col(resolution).astype(T)
        with np.errstate(divide="ignore"):
            self.inv_res = np.where(col(resolution) > 0, 1.0 / col(resolution), 0.0).astype(T)
        self.a, self.inv_dt = T(lowpass_gain(dt, tau_diff)), T(1.0 / dt)
        self.seed, self.rows = seed, np.arange(B, dtype=np.int64) + int(row_offset)
        self.counter = np.zeros(B, np.int32)
        self.ring = np.full((self.d + 1, B, width), np.nan, T)
        self.prev, self.d_f = np.full((B, width), np.nan, T), np.full((B, width), np.nan, T)
        self.v_hist = []

    def tick(self, x, n=None):
        """n: this tick's normals [B, W] when the caller has them already (normal_block), else they are drawn here"""
        T, W, d = self.T, self.W, self.d
        x = np.asarray(x, dtype=T)
        t = np.maximum(self.counter, 0).astype(np.int64)
        v = x + self.bias
        noisy = self.sigma != 0
        if noisy.any():
            if n is None:
                n = normal(self.seed, self.rows[:, None], t[:, None], np.arange(W)[None, :])
            vn = _fma(np.broadcast_to(self.sigma, v.shape), n.astype(T), v, T)
            v = np.where(noisy, vn, v)
        scaled = v.astype(np.float64) * self.inv_res.astype(np.float64)
        self.v_hist.append(np.where(self.res > 0, scaled, np.nan))
        q = (np.rint(v * self.inv_res) * self.res).astype(T)
        v = np.where(self.res > 0, q, v).astype(T)
        out = v
        if d > 0:
            b = np.arange(self.B)
            self.ring[t % (d + 1), b] = v
            out = self.ring[np.maximum(t - d, 0) % (d + 1), b]
        dy = None
        if self.difference:
            first = (t == 0)[:, None]
            with np.errstate(invalid="ignore"):
                g = (out - self.prev) * self.inv_dt
                df = _fma(np.broadcast_to(self.a, g.shape), (g - self.d_f).astype(T), self.d_f, T)
            self.g = np.where(first, T(0), g)
            self.d_f = np.where(first, T(0), df).astype(T)
            self.prev = out.copy()
            dy = self.d_f.copy()
        self.counter = (t + 1).astype(np.int32)
        return out.copy(), dy
