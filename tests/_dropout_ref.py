"""numpy statement of llmrec_dropout_rows_f32's mask and values, written from the words of include/llmrec_hip.h (R12) alone, on top of
tests/_sampler_ref.philox4x32_10 (checked against Random123's known answers). It imports nothing from llmrec_amd.

As documented:
  key      k = seed ^ 0xD1B54A32D192ED03; key words (k low, k high).
  counter  (c >> 2, r, step low, (step high * 256 + tag) mod 2^32) for row r, column c; the element uses output word c & 3.
  keep     word >= T, T = llrint(p * 2^32) in double, clamped to [1, 2^32 - 1].
  values   kept: x * scale, scale = 1.0f / (1.0f - p), both fp32; dropped: +0.0f."""
import numpy as np

from tests._sampler_ref import philox4x32_10

KEY_XOR = 0xD1B54A32D192ED03
TAG_ITEM_STREAMS, TAG_USER_PROFILE = 0, 1


def threshold(p):
    """T: the double product p * 2^32 rounded to the nearest integer (ties to even, llrint's default mode), clamped."""
    t = int(np.rint(np.float64(np.float32(p)) * np.float64(4294967296.0)))
    return min(max(t, 1), 2 ** 32 - 1)


def scale(p):
    """The fp32 quotient 1.0f / (1.0f - p)."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def words(rows, cols, seed, step, tag):
    """The 32-bit word of every element of a [rows, cols] tensor: uint32 [rows, cols]."""
    k = (int(seed) & (2 ** 64 - 1)) ^ KEY_XOR
    step = int(step) & (2 ** 64 - 1)
    groups = (cols + 3) // 4
    r = np.arange(rows, dtype=np.uint64)[:, None]
    g = np.arange(groups, dtype=np.uint64)[None, :]
    c3 = ((step >> 32) * 256 + int(tag)) & 0xFFFFFFFF
    o = philox4x32_10(g, r, step & 0xFFFFFFFF, c3, k & 0xFFFFFFFF, k >> 32)          # four [rows, groups] arrays
    return np.stack(o, axis=-1).reshape(rows, 4 * groups)[:, :cols]


def keep_mask(rows, cols, p, seed, step, tag):
    """bool [rows, cols]: True where the element is kept."""
    return words(rows, cols, seed, step, tag) >= np.uint32(threshold(p))


def apply(x, p, seed, step, tag):
    """The dropped tensor of the fp32 array x [rows, cols]: kept x * scale (fp32, one rounding), dropped +0.0."""
    x = np.asarray(x, dtype=np.float32)
    keep = keep_mask(x.shape[0], x.shape[1], p, seed, step, tag)
    with np.errstate(all="ignore"):
        scaled = x * scale(p)
    return np.where(keep, scaled, np.float32(0.0)).astype(np.float32)
