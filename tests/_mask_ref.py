"""numpy statement (float64) of the fused step's feature masking and attribute restoration, written from include/llmrec_hip.h (R13) on top
of tests/_sampler_ref.keyed_perm. It imports nothing from llmrec_amd.

As documented there:
  node lists   nodes[j] = keyed_perm(j, N) under the key seed ^ K_MASK with the step word (2 round + side) mod 2^64; side 0 = users, 1 = items.
  column sums  row lane j of ROW_LANES = 8 adds rows j, j + 8, ... in ascending order in fp64 from +0.0; the eight lanes are added in ascending j.
  a round      mean = fp32(sum / N); old = the listed rows' values in the same tree over the LIST POSITIONS; the listed rows become mean;
               sum = sum + (m * mean - old), every operation rounded once in fp64.
  restoration  y = W x + b; sce: mean_r (1 - cos(y_r, t_r))^alpha; mse: F.mse_loss(normalize(y), normalize(t)), eps 1e-12 as F.normalize;
               the gradient with respect to the rows x_r, times `scale`, added into the destination rows.

BOUNDS (u = 2^-24 for fp32, 2^-53 for fp64), each derived from the kernel's own order of operations:
  running sums   |device - exact| <= adds x 2^-53 x mag per column, where `adds` counts every fp64 operation the column's value has
                 passed through - N for a from-scratch sum (N - 1 additions, rounded up), m + 3 per round (m - 1 additions of old
                 values, the product, the difference, the update) - and `mag` is the sum of the magnitudes of everything that entered:
                 the |x| of the from-scratch sum, and per round the |old values|, m |mean| and |sum|. (Every partial result is bounded
                 by mag, and each operation rounds once: error <= adds x u x mag to first order; adds x u < 2^-30 here, so the second
                 order is below 2^-30 of the bound, covered by counting N for N - 1.) The fp32 mean adds nothing: the sum follows the
                 rounded value it stores. RunningBound keeps both numbers.
  stored mean    fp32(fp64(sum / N)) of a running sum within its bound b of the exact one: |stored - exact mean| <= b / N +
                 (2^-24 + 2 x 2^-53)(|exact mean| + b / N) - the sum's error, the quotient's rounding, the store's (stored_mean_bound).
  restoration    exact fp32 MFMA chains (v_mfma_f32_16x16x4_f32 = an fma chain, one rounding per product: dense.hip / _dense_ref.py):
                 an fma chain of n terms started from 0 has |error| <= n u sum|a_i b_i| to first order. Err below carries (value, absolute
                 error bound) through the kernel's formulas: + - * propagate both operands' bounds INCLUDING the second-order product
                 and add u |result| for the rounding; / and sqrt add 2 u |result| (one ulp: correctly rounded is better) with the
                 operand's bound propagated through the exact interval; the chains enter with n u S:
                   y[f]        64 products + the bias: 65 u (sum_k |W[f][k] x[k]| + |b[f]|)
                   yy, yt, tt  per lane 4 ceil(F / 16) fma's, then two additions: depth 4 ceil(F / 16) + 2
                   p[k], q[k]  16 ceil(F / 16) fma's over f (the tile's tail adds exact zeros)
                   loss_out    the 1024-slot tree: at most ceil(m / 1024) + 10 additions per term, then / m
                 A row whose norm is within its bound of eps has no bound (inf): the branch is not decidable; the cases avoid it."""
import numpy as np

from tests._sampler_ref import keyed_perm

K_MASK = 0x6A09E667F3BCC908
SIDE_USERS, SIDE_ITEMS = 0, 1
ROW_LANES = 8
U32, U64 = 2.0 ** -24, 2.0 ** -53
EPS = float(np.float32(1e-12))


def nodes(N, m, seed, rnd, side):
    """int64 [m]: the masked ids of round `rnd` on `side`."""
    seed = (int(seed) & (2 ** 64 - 1)) ^ K_MASK
    word = (2 * int(rnd) + int(side)) & (2 ** 64 - 1)
    return keyed_perm(np.arange(m, dtype=np.uint64), N, seed, word).astype(np.int64)


def lane_tree_sum(v):
    """fp64 [cols]: the sum over axis 0 of v [n, cols] in the documented tree (numpy's float64 + is the device's: one rounding)."""
    v = np.asarray(v, dtype=np.float64)
    lanes = np.zeros((ROW_LANES,) + v.shape[1:], dtype=np.float64)
    for i in range(v.shape[0]):
        lanes[i % ROW_LANES] = lanes[i % ROW_LANES] + v[i]
    s = lanes[0]
    for j in range(1, ROW_LANES):
        s = s + lanes[j]
    return s


def col_sums(X):
    return lane_tree_sum(np.asarray(X, dtype=np.float32))


def mask_round(X, sums, node_list, planted=None):
    """One round on the fp32 matrix X [N, cols] with the running sums [cols] -> (X', sums', mean fp32 [cols]).
    planted="sum_first": the defect of updating the sum before the mean is taken (the stored mean then comes from the NEW sum)."""
    X = np.array(X, dtype=np.float32)
    sums = np.asarray(sums, dtype=np.float64)
    N, m = X.shape[0], len(node_list)
    old = lane_tree_sum(X[node_list]) if m else np.zeros(X.shape[1])
    mean = (sums / np.float64(N)).astype(np.float32)
    put = np.float64(m) * mean.astype(np.float64)
    new = sums + (put - old)
    if planted == "sum_first":                                        # the rows get the mean of the sum that already counts them
        mean = (new / np.float64(N)).astype(np.float32)
    X[node_list] = mean
    return X, new, mean


class RunningBound:
    """adds and mag of a column's running sum (see BOUNDS)."""
    def __init__(self, X):
        X = np.abs(np.asarray(X, dtype=np.float64))
        self.adds, self.mag = X.shape[0], X.sum(0)

    def round(self, old_rows, mean, sums_before):
        m = old_rows.shape[0]
        self.adds += m + 3
        self.mag = self.mag + np.abs(old_rows.astype(np.float64)).sum(0) + m * np.abs(mean.astype(np.float64)) + np.abs(sums_before)

    def bound(self):
        return self.adds * U64 * self.mag

    def stored_mean_bound(self, N, mean):
        """|stored fp32 mean - mean| per column for the round that reads the sums as they stand (call it BEFORE round()); mean = the exact
        column mean of the tensor. The stored value is fp32(fp64(sum / N)) of a running sum within bound() of the exact one: the sum's
        error over N, then one fp64 rounding (the quotient) and one fp32 rounding (the store) of a value of at most |mean| + bound() / N."""
        e = self.bound() / N
        return e + (U32 + 2.0 * U64) * (np.abs(np.asarray(mean, dtype=np.float64)) + e)


# ------------------------------------------------------------------------------------------------------------------------------------
# restoration: the exact value and gradient
# ------------------------------------------------------------------------------------------------------------------------------------
def restore(X, T, node_list, W, b, loss_type, alpha, scale=1.0, eps=EPS, planted=None):
    """float64: {"row_loss" [m], "loss", "grad" [m, d] = scale dL/dx_r} for the rows X[node_list] [., d] against T[node_list] [., F].
    Written through the normalised vectors and the Jacobian of x / max(|x|, eps), not through the kernel's two coefficients.
    planted="no_c": the defect of dropping c = cos from t - c y in the cosine's gradient."""
    x, t = np.asarray(X, np.float64)[node_list], np.asarray(T, np.float64)[node_list]
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    m, F = t.shape
    y = x @ W.T + b
    ry, rt = np.sqrt((y * y).sum(1)), np.sqrt((t * t).sum(1))
    ny, nt = np.maximum(ry, eps), np.maximum(rt, eps)
    yh, th = y / ny[:, None], t / nt[:, None]
    free = (ry >= eps).astype(np.float64)[:, None]                    # 1: the norm moves with y; 0: clamped, dyh/dy = I / eps
    if loss_type == "sce":
        cos = (yh * th).sum(1)
        row = (1.0 - cos) ** alpha
        dcos = -alpha * (1.0 - cos) ** (alpha - 1.0) / m if alpha != 1 else np.full(m, -1.0 / m)
        g_yh = dcos[:, None] * th                                     # dL/dyh
    else:
        row = ((yh - th) ** 2).sum(1) / F
        g_yh = 2.0 * (yh - th) / (m * F)
    inner = (yh * g_yh).sum(1)[:, None]
    if planted == "no_c":                                             # yh . g_yh with cos replaced by 1
        inner = dcos[:, None] if loss_type == "sce" else inner * 0.0
    dy = (g_yh - free * yh * inner) / ny[:, None]
    return {"row_loss": row, "loss": row.mean(), "grad": scale * (dy @ W)}


# ------------------------------------------------------------------------------------------------------------------------------------
# restoration: the kernel's error bound
# ------------------------------------------------------------------------------------------------------------------------------------
class Err:
    """A float64 value with an absolute bound on what fp32 arithmetic in the kernel's order may have made of it."""
    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape).copy()

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(x)

    def _r(self, k=1.0):
        self.e = self.e + k * U32 * (np.abs(self.v) + self.e)
        return self

    def __add__(self, o):
        o = Err.of(o)
        return Err(self.v + o.v, self.e + o.e)._r()

    def __sub__(self, o):
        o = Err.of(o)
        return Err(self.v - o.v, self.e + o.e)._r()

    def __rsub__(self, o):
        return Err.of(o) - self

    def __neg__(self):
        return Err(-self.v, self.e)

    def __mul__(self, o):
        o = Err.of(o)
        return Err(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)._r()

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Err.of(o)
        with np.errstate(divide="ignore", invalid="ignore"):
            room = np.abs(o.v) - o.e
            q = self.v / o.v
            e = np.where(room > 0, (self.e + np.abs(q) * o.e) / np.where(room > 0, room, 1.0), np.inf)
        return Err(q, e)._r(2.0)

    def __rtruediv__(self, o):
        return Err.of(o) / self

    def sqrt(self):
        v = np.sqrt(self.v)
        lo, hi = np.sqrt(np.maximum(self.v - self.e, 0.0)), np.sqrt(self.v + self.e)
        return Err(v, np.maximum(v - lo, hi - v))._r(2.0)

    def clamp_min(self, c):
        return Err(np.maximum(self.v, c), self.e)                     # 1-Lipschitz, exact

    def ipow(self, n):
        out = self
        for _ in range(int(n) - 1):
            out = out * self
        return out


def fma_chain(A, B, n, eA=None):
    """Err of sum_i A[..., i] B[..., i] over the last axis as an fp32 fma chain of depth n; eA: bounds on A's entries (B exact)."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    eA = np.zeros_like(A) if eA is None else eA
    S = ((np.abs(A) + eA) * np.abs(B)).sum(-1)
    return Err((A * B).sum(-1), (eA * np.abs(B)).sum(-1) + n * U32 * S)


def restore_bound(X, T, node_list, W, b, loss_type, alpha, scale=1.0, dst0=None):
    """{"row_loss" [m], "loss", "grad" [m, d]}: bounds on |device - restore(...)| (grad: of the destination rows after the update, which
    held dst0 [m, d] before). alpha: 1, 2 or 3."""
    assert float(alpha) in (1.0, 2.0, 3.0)
    x, t = np.asarray(X, np.float64)[node_list], np.asarray(T, np.float64)[node_list]
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    m, F = t.shape
    tiles = -(-F // 16)
    y64 = x @ W.T + b
    ey = 65 * U32 * (np.abs(x) @ np.abs(W).T + np.abs(b))
    lane = 4 * tiles + 2
    syy = fma_chain(y64, y64, lane, ey)
    syy.e = syy.e + (ey * (np.abs(y64) + ey)).sum(1)                   # both factors carry ey
    syt, stt = fma_chain(y64, t, lane, ey), fma_chain(t, t, lane)
    p = fma_chain(y64[:, None, :], W.T[None, :, :], 16 * tiles, ey[:, None, :])      # [m, d]
    q = fma_chain(t[:, None, :], W.T[None, :, :], 16 * tiles)
    ry, rt = syy.sqrt(), stt.sqrt()
    undecided = np.abs(ry.v - EPS) <= ry.e
    ny, nt = ry.clamp_min(EPS), rt.clamp_min(EPS)
    nn = ny * nt
    cos, ny2 = syt / nn, ny * ny
    free = ry.v >= EPS
    fm = float(m)
    if loss_type == "sce":
        base = 1.0 - cos
        row = base.ipow(alpha)
        g = (float(alpha) * (Err(np.ones(m)) if alpha == 1 else base.ipow(alpha - 1))) / fm
        ca = -(g / nn)
        cb_free = g * cos / ny2
        cb = Err(np.where(free, cb_free.v, 0.0), np.where(free, cb_free.e, 0.0))
    else:
        row = ((syy / ny2 + stt / (nt * nt)) - 2.0 * cos) / float(F)
        g = Err(np.full(m, 2.0 / (fm * F)))._r()
        ca = -(g / nn)
        a_, b_ = g * cos, g
        cb = Err(np.where(free, a_.v, b_.v), np.where(free, a_.e, b_.e)) / ny2
    col = lambda z: Err(z.v[:, None], z.e[:, None])
    caq = col(ca) * q
    inner = col(cb) * p
    s = inner + caq                                                  # fmaf(cb, p, ca q) rounds cb p once less than this: the safe side
    grad = Err(np.full(1, float(scale))) * s
    d0 = np.zeros_like(grad.v) if dst0 is None else np.asarray(dst0, np.float64)
    after = Err(d0) + grad
    depth = -(-m // 1024) + 10
    loss_e = (row.e.sum() + depth * U32 * (np.abs(row.v) + row.e).sum()) / m + 2 * U32 * abs(row.v.mean())
    out = {"row_loss": row.e, "loss": loss_e, "grad": after.e}
    for k in ("row_loss", "grad"):
        out[k] = np.where(undecided.reshape((-1,) + (1,) * (out[k].ndim - 1)), np.inf, out[k])
    if undecided.any():
        out["loss"] = np.inf
    return out


def restore_fp32(X, T, node_list, W, b, loss_type, alpha, scale=1.0, dst0=None):
    """An fp32 emulation in ANOTHER order (numpy's float32 matrix products and pairwise sums): what tests/test_mask_ref_cpu.py holds below
    half the bounds."""
    f = np.float32
    x, t = np.asarray(X, f)[node_list], np.asarray(T, f)[node_list]
    W, b = np.asarray(W, f), np.asarray(b, f)
    m, F = t.shape
    y = x @ W.T + b
    syy, syt, stt = (y * y).sum(1), (y * t).sum(1), (t * t).sum(1)
    ry, rt = np.sqrt(syy), np.sqrt(stt)
    ny, nt = np.maximum(ry, f(EPS)), np.maximum(rt, f(EPS))
    cos = syt / (ny * nt)
    if loss_type == "sce":
        base = f(1) - cos
        row = base ** int(alpha)
        g = f(alpha) * (base ** int(alpha - 1) if alpha != 1 else f(1)) / f(m)
        ca, cb = -(g / (ny * nt)), np.where(ry >= f(EPS), g * cos / (ny * ny), f(0))
    else:
        row = (syy / (ny * ny) + stt / (nt * nt) - f(2) * cos) / f(F)
        g = f(2) / (f(m) * f(F))
        ca, cb = -(g / (ny * nt)), np.where(ry >= f(EPS), g * cos, g) / (ny * ny)
    grad = f(scale) * (cb[:, None] * (y @ W) + ca[:, None] * (t @ W))
    d0 = np.zeros_like(grad) if dst0 is None else np.asarray(dst0, f)
    return {"row_loss": row, "loss": row.sum(dtype=f) / f(m), "grad": d0 + grad}
