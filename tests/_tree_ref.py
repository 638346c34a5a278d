"""float32 restatements (numpy, CPU) of the loss kernels' fixed-order sums: the 1024-slot pairwise tree of bpr_reduce_kernel /
block_tree_sum, and the same tree as ONE wavefront walks it in llmrec_bpr_multi_losses_assemble_f32 (16 registers per lane, then
shuffles). Both add float32 values one addition at a time, so their bits are the kernels' bits."""
import numpy as np

SLOTS = 1024


def slot_sums(x):
    """slot v = x[v] + x[v + 1024] + ... in ascending order, started from 0.f"""
    x = np.asarray(x, dtype=np.float32)
    red = np.zeros(SLOTS, dtype=np.float32)
    for b0 in range(0, len(x), SLOTS):
        chunk = x[b0:b0 + SLOTS]
        red[:len(chunk)] = red[:len(chunk)] + chunk                     # one float32 addition per slot, ascending b
    return red


def tree_lds(x):
    """the 1024-slot tree: red[i] += red[i + off] for i < off, off = 512 ... 1"""
    red = slot_sums(x).copy()
    off = SLOTS // 2
    while off > 0:
        red[:off] = red[:off] + red[off:2 * off]
        off >>= 1
    return red[0]


def tree_wave(x):
    """one wavefront: lane l holds slots l + 64 j in r[j]; levels 512 ... 64 are r[j] += r[j + off / 64]; levels 32 ... 1 are
    x += shfl_down(x, off) in EVERY lane (a lane whose source is past the wavefront reads its own value, as the hardware does)"""
    r = slot_sums(x).reshape(16, 64).copy()                             # r[j][l] = slot l + 64 j
    h = 8
    while h > 0:
        r[:h] = r[:h] + r[h:2 * h]
        h >>= 1
    v = r[0].copy()
    off = 32
    with np.errstate(over="ignore", invalid="ignore"):
        while off > 0:
            src = np.arange(64) + off
            src = np.where(src < 64, src, np.arange(64))
            v = v + v[src]
            off >>= 1
    return v[0]
