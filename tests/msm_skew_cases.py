"""Shared by the tests of the split of overlong bucket runs (tests/test_msm_split_emul.py,
tests/test_gpu_msm_skew.py, tests/test_gpu_msm_g2_skew.py): skewed scalar patterns for a
multi-scalar multiplication over either group and their expected values from the oracle
alone -- O.g*_mul, a halving tree of O.g*_add, O.g*_normalize; a zero sum is the
(0, one, 0) image.  Where many terms share a scalar the expected value uses
sum k * P_i = k * sum P_i, one oracle multiplication of the oracle's tree sum."""
import numpy as np

from oracle import oracle as O

R = O.R
NT = 16
PATTERNS = ["a_equal", "b_ones", "b_minus_ones", "c_repeated", "d_cancelling", "e_zero_images", "f_two_hot",
            "g_top_bits"]
# one random scalar; a scalar with both top bits (253, 252) set, below r = 0x3064...
K_EQUAL = 0x1f2e3d4c5b6a79880123456789abcdef0fedcba987654321a5a5a5a55a5a5a5a % R
K_TOP = (3 << 252) | 0x123456789abcdef0fedcba9876543210123456789abcdef
K_HOT = (0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe % R, R - 0x31415926535897932384626433832795)
assert K_TOP < R


class Group:
    def __init__(self, name):
        self.name = name
        self.width = {"g1": 12, "g2": 24}[name]
        self.mul = {"g1": O.g1_mul, "g2": O.g2_mul}[name]
        self.add = {"g1": O.g1_add, "g2": O.g2_add}[name]
        self.neg = {"g1": O.g1_neg, "g2": O.g2_neg}[name]
        self.normalize = {"g1": O.g1_normalize, "g2": O.g2_normalize}[name]
        one = O.canon_to_mont_array([1]).reshape(4)
        z = np.zeros(self.width, np.uint64)
        z[self.width // 3:self.width // 3 + 4] = one
        self._zero = z

    def zero(self):
        return self._zero.copy()

    def points(self, n, seed):
        """n Jacobian images (z != one) of random multiples of the generator."""
        one = {"g1": O.g1_one, "g2": O.g2_one}[self.name]()
        _, s = O.random_scalars(n, seed)
        return self.mul(one, s, NT)

    def tree(self, a):
        a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, self.width).copy()
        while a.shape[0] > 1:
            h = (a.shape[0] + 1) // 2
            m = a.shape[0] - h
            a[:m] = self.add(a[:m], a[h:])
            a = a[:h]
        return a

    def image(self, a):
        """The returned image of the Jacobian point(s) a[0:1]; no point: zero."""
        if a.shape[0] == 0:
            return self.zero()
        r = self.normalize(a[:1])[0]
        return r if r[2 * self.width // 3:].any() else self.zero()

    def times(self, a, k):
        """k * (the tree sum of the points a), as a (1, width) Jacobian image."""
        if a.shape[0] == 0:
            return a.reshape(0, self.width)
        return self.mul(self.tree(a), fr([k]), 1)


def fr(vals):
    return O.canon_to_mont_array([v % R for v in vals], O.FR).reshape(len(vals), 4)


def same(k, n):
    return np.ascontiguousarray(np.broadcast_to(fr([k])[0], (n, 4)))


def case(g, pattern, pts, uni_k, uni_prod):
    """(points, scalars, expected image) of `pattern` over the n points pts; uni_k / uni_prod:
    n uniform scalars and the oracle's products pts[i] * uni_k[i] (pattern f's uniform half)."""
    n = pts.shape[0]
    if pattern == "a_equal":
        return pts, same(K_EQUAL, n), g.image(g.times(pts, K_EQUAL))
    if pattern == "b_ones":
        return pts, same(1, n), g.image(g.tree(pts))
    if pattern == "b_minus_ones":     # negative digits: the sign bit of the entries on the chunk path
        return pts, same(R - 1, n), g.image(g.neg(g.tree(pts)))
    if pattern == "c_repeated":       # equal chunk sums: every fold level takes jac_add's doubling branch
        p = np.ascontiguousarray(np.broadcast_to(pts[n // 2], (n, g.width)))
        return p, same(K_EQUAL, n), g.image(g.mul(pts[n // 2:n // 2 + 1], fr([K_EQUAL * n]), 1))
    if pattern == "d_cancelling":     # P, -P alternating: chunk sums may be zero
        p = np.ascontiguousarray(np.broadcast_to(pts[n // 2], (n, g.width))).copy()
        p[1::2] = g.neg(pts[n // 2:n // 2 + 1])[0]
        want = g.zero() if n % 2 == 0 else g.image(g.mul(pts[n // 2:n // 2 + 1], fr([K_EQUAL]), 1))
        return p, same(K_EQUAL, n), want
    if pattern == "e_zero_images":    # z = 0 under junk x, y, interleaved with pattern a
        p = pts.copy()
        p[1::2, 2 * g.width // 3:] = 0
        return p, same(K_EQUAL, n), g.image(g.times(pts[0::2], K_EQUAL))
    if pattern == "f_two_hot":        # half uniform, a third and a sixth on two hot values
        h, t = n // 2, n // 2 + n // 3
        k = uni_k.copy()
        k[h:t] = fr([K_HOT[0]])[0]
        k[t:] = fr([K_HOT[1]])[0]
        parts = [g.tree(uni_prod[:h]), g.times(pts[h:t], K_HOT[0]), g.times(pts[t:], K_HOT[1])]
        return pts, k, g.image(g.tree(np.concatenate([a for a in parts if a.shape[0]])))
    if pattern == "g_top_bits":       # the top window's replica buckets
        return pts, same(K_TOP, n), g.image(g.times(pts, K_TOP))
    raise ValueError(pattern)


# ---- the GPU side (tests/test_gpu_msm_skew.py, tests/test_gpu_msm_g2_skew.py)
CAPS = [1, 3, 64, 0, "unsplit"]   # bn_set_msm_run_max: forced caps, the default rule, never split
WINDOWS = [2, 5, 16, 0]           # bn_set_msm_window; 0: automatic


def set_cap(ctx, cap):
    from substrate_bn import _native
    ctx.set_msm_run_max(_native.MSM_RUN_UNSPLIT if cap == "unsplit" else cap)


def all_settings(ctx, group, p, k, windows=WINDOWS, caps=CAPS):
    """{(c, cap): image} of the same MSM on the bucket path (bn_set_msm_min(0)) by the host
    form at every window width and run cap; the context is left at its defaults."""
    msm = {"g1": ctx.g1_msm, "g2": ctx.g2_msm}[group]
    got = {}
    try:
        ctx.set_msm_min(0)
        for c in windows:
            ctx.set_msm_window(c)
            for cap in caps:
                set_cap(ctx, cap)
                got[(c, cap)] = msm(p, k)
    finally:
        ctx.set_msm_window(0)
        ctx.set_msm_run_max(0)
    return got


def dev_form(ctx, group, p, k):
    """The image by the device-pointer form on the context's stream at the current settings."""
    import torch
    dev = torch.device("cuda", 0)
    w = {"g1": 12, "g2": 24}[group]
    n = p.shape[0]
    P = torch.from_numpy(np.array(p, dtype=np.uint64).view(np.int64).reshape(-1)).to(dev)
    K = torch.from_numpy(np.array(k, dtype=np.uint64).view(np.int64).reshape(-1)).to(dev)
    out = torch.full((w,), 0x5a5a, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)  # the context's own stream is not ordered after torch's
    {"g1": ctx.g1_msm_dev, "g2": ctx.g2_msm_dev}[group](P.data_ptr(), K.data_ptr(), n, out.data_ptr())
    ctx.dev_status()  # synchronizes the context's stream
    return out.cpu().numpy().view(np.uint64)
