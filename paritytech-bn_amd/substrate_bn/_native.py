"""ctypes binding of libbn254mi.so (include/bn254mi.h).

The product path: every call runs the HIP kernels on an MI355X.  There is no
CPU fallback -- if the library or a GPU is missing the calls raise.
Arrays are numpy uint64 in the reference memory image:
  G1 (n, 12), G2 (n, 24), Gt (n, 48), Fr (n, 4).
"""
import ctypes
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("BN254MI_LIB") or os.path.join(PKG_DIR, "libbn254mi.so")  # override: A/B builds

BN_OK = 0
BN_ERR_INVALID_ARGUMENT = 1
BN_ERR_TO_AFFINE = 2
BN_ERR_FE_ZERO = 3
BN_ERR_HIP = 4
BN_ERR_NO_DEVICE = 5
BN_ERR_INTERNAL = 6

FQ12_OPS = {"mul": 0, "sqr": 1, "inv": 2, "cyc_sqr": 3, "exp_by_neg_z": 4, "frob1": 5, "frob2": 6, "frob3": 7}

# every symbol include/bn254mi.h declares (checked by tests/test_capi_symbols.py)
EXPORTS = [
    "bn_ctx_create", "bn_ctx_destroy", "bn_last_error", "bn_ctx_stream",
    "bn_pairing_many", "bn_pairing_many_dev", "bn_pairing_batch", "bn_miller_loop_batch",
    "bn_final_exponentiation_many", "bn_miller_loop_many",
    "bn_g1_mul_many", "bn_g1_mul_many_dev", "bn_g2_mul_many", "bn_g2_mul_many_dev",
    "bn_fq12_op_many", "bn_workspace_bytes", "bn_reserve", "bn_set_phase_timing", "bn_get_phase_times",
    "bn_fq_from_slice_many", "bn_fq_to_big_endian_many", "bn_fq2_from_slice_many", "bn_fr_from_slice_many",
    "bn_fr_to_big_endian_many", "bn_fq_sqrt_many", "bn_fq2_sqrt_many", "bn_g1_affine_new_many",
    "bn_g2_affine_new_many", "bn_g2_affine_new_many_dev", "bn_g1_from_compressed_many", "bn_g2_from_compressed_many",
    "bn_g1_from_compressed_many_dev", "bn_g2_from_compressed_many_dev", "bn_gt_pow_many", "bn_gt_pow_many_dev",
    "bn_ctx_create_multi", "bn_ctx_num_devices", "bn_ctx_device", "bn_shard_range", "bn_pairing_many_allgather_dev",
    "bn_pairing_batch_dev", "bn_miller_loop_batch_dev", "bn_set_fe_wide_max", "bn_g2_precompute_many",
    "bn_set_latency_max", "bn_dev_status", "bn_set_fq12_op_unit",
    "bn_g1_msm", "bn_g1_msm_dev", "bn_set_msm_window", "bn_set_msm_min", "bn_msm_reserve",
    "bn_set_msm_run_max",
    "bn_g2_msm", "bn_g2_msm_dev", "bn_g2_msm_reserve",
    "bn_g1_prepared_table_bytes", "bn_g1_bases_prepare", "bn_g1_bases_prepare_dev", "bn_g1_prepared_count",
    "bn_g1_prepared_window", "bn_g1_prepared_destroy", "bn_g1_msm_prepared_many", "bn_g1_msm_prepared_many_dev",
    "bn_set_msm_prepared_lanes",
    "bn_g1_msm_many", "bn_g1_msm_many_dev", "bn_set_msm_many_window", "bn_set_msm_many_unit", "bn_set_msm_many_max",
    "bn_set_msm_many_chunk", "bn_g1_msm_many_reserve",
    "bn_g1_basis_table_bytes", "bn_g1_basis_prepare", "bn_g1_basis_prepare_dev", "bn_g1_basis_count",
    "bn_g1_basis_window", "bn_g1_basis_destroy", "bn_g1_msm_basis", "bn_g1_msm_basis_dev", "bn_g1_msm_basis_reserve",
    "bn_g1_msm_basis_many", "bn_g1_msm_basis_many_dev", "bn_g1_msm_basis_many_reserve", "bn_set_msm_basis_many_set",
    "bn_g2_basis_table_bytes", "bn_g2_basis_prepare", "bn_g2_basis_prepare_dev", "bn_g2_basis_count",
    "bn_g2_basis_window", "bn_g2_basis_destroy", "bn_g2_msm_basis", "bn_g2_msm_basis_dev", "bn_g2_msm_basis_reserve",
    "bn_pairing_batch_many", "bn_pairing_batch_many_dev", "bn_set_products_min", "bn_set_products_chunk",
    "bn_set_products_wide_max", "bn_get_products_routes",
    "bn_g2_prepare", "bn_g2_prepare_dev", "bn_g2_prepared_count", "bn_g2_prepared_destroy",
    "bn_pairing_prepared_many", "bn_pairing_prepared_many_dev", "bn_miller_loop_prepared_many",
    "bn_pairing_batch_prepared_many", "bn_pairing_batch_prepared_many_dev",
] + ["bn_%s_%s_many%s" % (g, op, dev) for g in ("g1", "g2") for op in ("add", "sub", "neg", "normalize", "eq")
     for dev in ("", "_dev")]
GROUP_OPS = ("add", "sub", "neg", "normalize", "eq")

# per-element status (bn_elem_status)
ST_OK, ST_FIELD_INVALID_SLICE_LENGTH, ST_FIELD_INVALID_U512, ST_FIELD_NOT_MEMBER = 0, 1, 2, 3
ST_CURVE_INVALID_ENCODING, ST_CURVE_NOT_MEMBER, ST_GROUP_NOT_ON_CURVE, ST_GROUP_NOT_IN_SUBGROUP = 4, 5, 6, 7


class BnError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("bn254mi error %d: %s" % (code, msg))
        self.code = code


_lib = None


def load():
    """Load the native library (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libbn254mi.so not built: run `make -C paritytech-bn_amd` "
                          "(or __graft_entry__.build())")
    # One HIP runtime per process: torch ships its own libamdhip64.so.7 (and HSA
    # runtime).  Loaded first, it satisfies this library's libamdhip64.so.7 by
    # SONAME, so engine calls and torch tensors/streams/RCCL share one runtime;
    # loaded the other way round the process would hold two runtimes.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, sz, i, u8p = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p
    sig = {
        "bn_ctx_create": ([i, ctypes.POINTER(vp)], i),
        "bn_ctx_destroy": ([vp], i),
        "bn_last_error": ([vp], ctypes.c_char_p),
        "bn_ctx_stream": ([vp], vp),
        "bn_pairing_many": ([vp, vp, vp, sz, vp], i),
        "bn_pairing_many_dev": ([vp, vp, vp, sz, vp, vp], i),
        "bn_pairing_batch": ([vp, vp, vp, sz, vp], i),
        "bn_miller_loop_batch": ([vp, vp, vp, sz, vp], i),
        "bn_final_exponentiation_many": ([vp, vp, sz, vp, u8p], i),
        "bn_miller_loop_many": ([vp, vp, vp, sz, vp], i),
        "bn_g1_mul_many": ([vp, vp, vp, sz, vp], i),
        "bn_g1_mul_many_dev": ([vp, vp, vp, sz, vp, vp], i),
        "bn_g2_mul_many": ([vp, vp, vp, sz, vp], i),
        "bn_g2_mul_many_dev": ([vp, vp, vp, sz, vp, vp], i),
        "bn_fq12_op_many": ([vp, i, vp, vp, sz, vp], i),
        "bn_workspace_bytes": ([sz], sz),
        "bn_reserve": ([vp, sz], i),
        "bn_set_phase_timing": ([vp, i], i),
        "bn_get_phase_times": ([vp, vp, vp], i),
        "bn_fq_from_slice_many": ([vp, vp, sz, vp, vp], i),
        "bn_fq_to_big_endian_many": ([vp, vp, sz, vp], i),
        "bn_fq2_from_slice_many": ([vp, vp, sz, vp, vp], i),
        "bn_fr_from_slice_many": ([vp, vp, sz, vp], i),
        "bn_fr_to_big_endian_many": ([vp, vp, sz, vp], i),
        "bn_fq_sqrt_many": ([vp, vp, sz, vp, vp], i),
        "bn_fq2_sqrt_many": ([vp, vp, sz, vp, vp], i),
        "bn_g1_affine_new_many": ([vp, vp, vp, sz, vp, vp], i),
        "bn_g2_affine_new_many": ([vp, vp, vp, sz, vp, vp], i),
        "bn_g2_affine_new_many_dev": ([vp, vp, vp, sz, vp, vp, vp], i),
        "bn_g1_from_compressed_many": ([vp, vp, sz, vp, vp], i),
        "bn_g2_from_compressed_many": ([vp, vp, sz, vp, vp], i),
        "bn_g1_from_compressed_many_dev": ([vp, vp, sz, vp, vp, vp], i),
        "bn_g2_from_compressed_many_dev": ([vp, vp, sz, vp, vp, vp], i),
        "bn_gt_pow_many": ([vp, vp, vp, sz, vp], i),
        "bn_gt_pow_many_dev": ([vp, vp, vp, sz, vp, vp], i),
        "bn_ctx_create_multi": ([vp, i, ctypes.POINTER(vp)], i),
        "bn_ctx_num_devices": ([vp], i),
        "bn_ctx_device": ([vp, i], vp),
        "bn_shard_range": ([sz, i, i, ctypes.POINTER(sz), ctypes.POINTER(sz)], None),
        "bn_pairing_many_allgather_dev": ([vp, vp, vp, sz, vp, vp], i),
        "bn_pairing_batch_dev": ([vp, vp, vp, sz, vp, vp, vp], i),
        "bn_miller_loop_batch_dev": ([vp, vp, vp, sz, vp, vp, vp], i),
        "bn_set_fe_wide_max": ([vp, sz], i),
        "bn_set_latency_max": ([vp, sz], i),
        "bn_set_fq12_op_unit": ([vp, i], i),
        "bn_g2_precompute_many": ([vp, vp, sz, vp], i),
        "bn_dev_status": ([vp, vp], i),
        "bn_g1_msm": ([vp, vp, vp, sz, vp], i),
        "bn_g1_msm_dev": ([vp, vp, vp, sz, vp, vp], i),
        "bn_set_msm_window": ([vp, i], i),
        "bn_set_msm_min": ([vp, sz], i),
        "bn_set_msm_run_max": ([vp, sz], i),
        "bn_msm_reserve": ([vp, sz], i),
        "bn_g2_msm": ([vp, vp, vp, sz, vp], i),
        "bn_g2_msm_dev": ([vp, vp, vp, sz, vp, vp], i),
        "bn_g2_msm_reserve": ([vp, sz], i),
        "bn_g1_prepared_table_bytes": ([sz, i], sz),
        "bn_g1_bases_prepare": ([vp, vp, sz, i, ctypes.POINTER(vp)], i),
        "bn_g1_bases_prepare_dev": ([vp, vp, sz, i, ctypes.POINTER(vp), vp], i),
        "bn_g1_prepared_count": ([vp], sz),
        "bn_g1_prepared_window": ([vp], i),
        "bn_g1_prepared_destroy": ([vp, vp], i),
        "bn_g1_msm_prepared_many": ([vp, vp, vp, sz, vp, sz], i),
        "bn_g1_msm_prepared_many_dev": ([vp, vp, vp, sz, vp, sz, vp], i),
        "bn_set_msm_prepared_lanes": ([vp, i], i),
        "bn_g1_msm_many": ([vp, vp, vp, vp, sz, vp, sz], i),
        "bn_g1_msm_many_dev": ([vp, vp, vp, vp, sz, vp, sz, vp], i),
        "bn_set_msm_many_window": ([vp, i], i),
        "bn_set_msm_many_unit": ([vp, i], i),
        "bn_set_msm_many_max": ([vp, sz], i),
        "bn_set_msm_many_chunk": ([vp, sz], i),
        "bn_g1_msm_many_reserve": ([vp, sz, sz], i),
        "bn_g1_basis_table_bytes": ([sz, i], sz),
        "bn_g1_basis_prepare": ([vp, vp, sz, i, ctypes.POINTER(vp)], i),
        "bn_g1_basis_prepare_dev": ([vp, vp, sz, i, ctypes.POINTER(vp), vp], i),
        "bn_g1_basis_count": ([vp], sz),
        "bn_g1_basis_window": ([vp], i),
        "bn_g1_basis_destroy": ([vp, vp], i),
        "bn_g1_msm_basis": ([vp, vp, vp, sz, vp], i),
        "bn_g1_msm_basis_dev": ([vp, vp, vp, sz, vp, vp], i),
        "bn_g1_msm_basis_reserve": ([vp, vp, sz], i),
        "bn_g1_msm_basis_many": ([vp, vp, vp, sz, sz, sz, vp, sz], i),
        "bn_g1_msm_basis_many_dev": ([vp, vp, vp, sz, sz, sz, vp, sz, vp], i),
        "bn_g1_msm_basis_many_reserve": ([vp, vp, sz, sz], i),
        "bn_set_msm_basis_many_set": ([vp, sz], i),
        "bn_g2_basis_table_bytes": ([sz, i], sz),
        "bn_g2_basis_prepare": ([vp, vp, sz, i, ctypes.POINTER(vp)], i),
        "bn_g2_basis_prepare_dev": ([vp, vp, sz, i, ctypes.POINTER(vp), vp], i),
        "bn_g2_basis_count": ([vp], sz),
        "bn_g2_basis_window": ([vp], i),
        "bn_g2_basis_destroy": ([vp, vp], i),
        "bn_g2_msm_basis": ([vp, vp, vp, sz, vp], i),
        "bn_g2_msm_basis_dev": ([vp, vp, vp, sz, vp, vp], i),
        "bn_g2_msm_basis_reserve": ([vp, vp, sz], i),
        "bn_pairing_batch_many": ([vp, vp, vp, vp, sz, vp], i),
        "bn_pairing_batch_many_dev": ([vp, vp, vp, vp, sz, vp, vp], i),
        "bn_set_products_min": ([vp, sz], i),
        "bn_set_products_chunk": ([vp, sz], i),
        "bn_set_products_wide_max": ([vp, sz], i),
        "bn_get_products_routes": ([vp, vp], i),
        "bn_g2_prepare": ([vp, vp, sz, ctypes.POINTER(vp)], i),
        "bn_g2_prepare_dev": ([vp, vp, sz, ctypes.POINTER(vp), vp], i),
        "bn_g2_prepared_count": ([vp], sz),
        "bn_g2_prepared_destroy": ([vp, vp], i),
        "bn_pairing_prepared_many": ([vp, vp, vp, vp, sz, vp], i),
        "bn_pairing_prepared_many_dev": ([vp, vp, vp, vp, sz, vp, vp], i),
        "bn_miller_loop_prepared_many": ([vp, vp, vp, vp, sz, vp], i),
        "bn_pairing_batch_prepared_many": ([vp, vp, vp, vp, vp, vp, sz, vp], i),
        "bn_pairing_batch_prepared_many_dev": ([vp, vp, vp, vp, vp, vp, sz, vp, vp], i),
    }
    for g in ("g1", "g2"):
        for op in GROUP_OPS:
            unary = op in ("neg", "normalize")
            sig["bn_%s_%s_many" % (g, op)] = ([vp, vp, sz, vp] if unary else [vp, vp, vp, sz, vp], i)
            sig["bn_%s_%s_many_dev" % (g, op)] = ([vp, vp, sz, vp, vp] if unary else [vp, vp, vp, sz, vp, vp], i)
    ab_build = bool(os.environ.get("BN254MI_LIB"))  # an A/B build may predate newer entry points
    for name, (args, res) in sig.items():
        if ab_build and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    _lib = L
    return L


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _arr(a, width):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.size % width:
        raise ValueError("array of %d words is not a multiple of %d" % (a.size, width))
    return a.reshape(-1, width)


def _same_rows(*arrays):
    """Row count shared by paired inputs; a mismatch raises before any native call
    (the C ABI reads n rows from every buffer)."""
    n = arrays[0].shape[0]
    for a in arrays[1:]:
        if a.shape[0] != n:
            raise ValueError("paired inputs have %d and %d rows" % (n, a.shape[0]))
    return n


def _offsets(offsets, n=None):
    """The m + 1 product offsets as a contiguous size_t array: non-decreasing from 0, and
    ending at n when the row count is known.  Anything else raises ValueError before any
    native call (the C ABI refuses it too)."""
    raw = np.asarray(offsets)
    if raw.ndim != 1 or raw.size == 0:
        raise ValueError("offsets must be a one-dimensional sequence of m + 1 entries")
    if raw.dtype.kind not in "iu":
        raise ValueError("offsets must be integers")
    if raw.dtype.kind == "i" and (raw < 0).any():
        raise ValueError("offsets must not be negative")
    off = np.ascontiguousarray(raw, dtype=np.uintp)
    if off[0] != 0:
        raise ValueError("offsets[0] must be 0, not %d" % int(off[0]))
    if (off[1:] < off[:-1]).any():
        raise ValueError("offsets must not decrease")
    if n is not None and int(off[-1]) != n:
        raise ValueError("offsets end at %d but there are %d pairs" % (int(off[-1]), n))
    return off


def _indices(idx, n, nq):
    """The n prepared-point indices as a contiguous uint32 array, or None (every pair takes
    point 0) when idx is None.  A wrong count, a negative index, one that is not an integer
    and one >= nq raise ValueError before any native call (the C ABI's host forms refuse the
    last too)."""
    if idx is None:
        return None
    raw = np.asarray(idx)
    if raw.ndim != 1 or raw.shape[0] != n:
        raise ValueError("idx must hold one index per pair (%d), not shape %s" % (n, raw.shape))
    if raw.dtype.kind not in "iu":
        raise ValueError("idx must be integers")
    if raw.dtype.kind == "i" and (raw < 0).any():
        raise ValueError("idx must not be negative")
    if n and int(raw.max()) >= nq:
        raise ValueError("idx holds %d but there are %d prepared points" % (int(raw.max()), nq))
    return np.ascontiguousarray(raw, dtype=np.uint32)


QIDX_FRESH = 0xffffffff   # BN_QIDX_FRESH: the term's G2 point is the next entry of q
MSM_RUN_UNSPLIT = ctypes.c_size_t(-1).value  # BN_MSM_RUN_UNSPLIT: bn_set_msm_run_max's "never split"
PRODUCT_LANE_MAX = 64     # terms per product of pairing_batch_prepared_many


def _term_indices(qidx, n, nq):
    """The n per-term words of pairing_batch_prepared_many as a contiguous uint32 array: each
    QIDX_FRESH or a prepared-point index < nq.  Anything else raises ValueError before any
    native call (the C ABI refuses it too).  Returns (array, number of fresh terms)."""
    raw = np.asarray(qidx)
    if raw.ndim != 1 or raw.shape[0] != n:
        raise ValueError("qidx must hold one entry per term (%d), not shape %s" % (n, raw.shape))
    if n and raw.dtype.kind not in "iu":
        raise ValueError("qidx must be integers")
    if n and raw.dtype.kind == "i" and (raw < 0).any():
        raise ValueError("qidx must not be negative")
    raw = raw.astype(np.uint64)
    fresh = raw == QIDX_FRESH
    if (~fresh & (raw >= nq)).any():
        raise ValueError("qidx holds %d but there are %d prepared points" % (int(raw[~fresh].max()), nq))
    return np.ascontiguousarray(raw, dtype=np.uint32), int(fresh.sum())


def _product_lengths(off):
    if off.shape[0] > 1 and int((off[1:] - off[:-1]).max()) > PRODUCT_LANE_MAX:
        raise ValueError("a product of more than %d terms; use pairing_batch" % PRODUCT_LANE_MAX)


def shard_range(n, ndev, k):
    """[lo, hi) of shard k of n elements over ndev devices (the C ABI's split)."""
    lo, hi = ctypes.c_size_t(), ctypes.c_size_t()
    load().bn_shard_range(n, ndev, k, ctypes.byref(lo), ctypes.byref(hi))
    return lo.value, hi.value


class Context:
    """One device context (bn_ctx), or with `devices=[...]` one context over several
    devices of the node (bn_ctx_create_multi).  All arrays are reference memory images."""

    def __init__(self, device=0, devices=None):
        L = load()
        h = ctypes.c_void_p()
        if devices is None:
            rc = L.bn_ctx_create(device, ctypes.byref(h))
        else:
            arr = (ctypes.c_int * len(devices))(*devices)
            rc = L.bn_ctx_create_multi(arr, len(devices), ctypes.byref(h))
        if rc != BN_OK:
            raise BnError(rc, "bn_ctx_create(%s) failed" % (device if devices is None else devices))
        self._h = h
        self._L = L

    @property
    def num_devices(self):
        return self._L.bn_ctx_num_devices(self._h)

    def pairing_many_allgather_dev(self, d_p, d_q, n_per_dev, d_out, streams=None):
        """Config 4 in one process: per-device pointer lists (ints); every d_out[k]
        receives all num_devices * n_per_dev results in device order."""
        nd = len(d_p)
        vp = ctypes.c_void_p
        arr = lambda xs: (vp * nd)(*xs)  # noqa: E731
        self._check(self._L.bn_pairing_many_allgather_dev(self._h, arr(d_p), arr(d_q), n_per_dev, arr(d_out),
                                                          arr(streams) if streams else None))

    def device(self, k):
        """Device k's single-device context of a multi-device context (bn_ctx_device):
        owned by this context, valid while it lives."""
        h = self._L.bn_ctx_device(self._h, k)
        if not h:
            raise BnError(BN_ERR_INVALID_ARGUMENT, "no device %d in this context" % k)
        sub = Context.__new__(Context)
        sub._h = ctypes.c_void_p(h)
        sub._L = self._L
        sub._owner = self  # keeps the parent (which destroys it) alive
        return sub

    def dev_status(self, stream=None):
        """bn_dev_status: synchronize and raise on the sticky device outcome of the
        status-less _dev calls (BN_ERR_INTERNAL, then BN_ERR_INVALID_ARGUMENT: a prepared-point
        index out of range, then BN_ERR_FE_ZERO); clears it."""
        self._check(self._L.bn_dev_status(self._h, stream))

    def close(self):
        if getattr(self, "_owner", None) is not None:  # a device of a multi-device context
            self._h = None
            return
        if getattr(self, "_h", None):
            self._L.bn_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != BN_OK:
            raise BnError(rc, (self._L.bn_last_error(self._h) or b"").decode())

    @property
    def handle(self):
        return self._h

    @property
    def stream(self):
        return self._L.bn_ctx_stream(self._h)

    # ---- group law (lib.rs:388-423, 539-574)
    def group_op_many(self, group, op, a, b=None):
        """bn_{g1,g2}_{add,sub,neg,normalize,eq}_many: rows of a (and b); eq returns a
        uint8 array, the others point images."""
        w = {"g1": 12, "g2": 24}[group]
        a = _arr(a, w)
        args = [self._h, _ptr(a)]
        if op not in ("neg", "normalize"):
            b = _arr(b, w)
            _same_rows(a, b)
            args.append(_ptr(b))
        out = np.zeros(a.shape[0], np.uint8) if op == "eq" else np.zeros((a.shape[0], w), np.uint64)
        self._check(getattr(self._L, "bn_%s_%s_many" % (group, op))(*args, a.shape[0], _ptr(out)))
        return out

    def group_op_many_dev(self, group, op, d_a, d_b, n, d_out, stream=None):
        fn = getattr(self._L, "bn_%s_%s_many_dev" % (group, op))
        if op in ("neg", "normalize"):
            self._check(fn(self._h, d_a, n, d_out, stream))
        else:
            self._check(fn(self._h, d_a, d_b, n, d_out, stream))

    # ---- pairing path
    def pairing_many(self, p, q):
        p, q = _arr(p, 12), _arr(q, 24)
        _same_rows(p, q)
        out = np.zeros((p.shape[0], 48), np.uint64)
        self._check(self._L.bn_pairing_many(self._h, _ptr(p), _ptr(q), p.shape[0], _ptr(out)))
        return out

    def pairing_batch(self, p, q):
        p, q = _arr(p, 12), _arr(q, 24)
        _same_rows(p, q)
        out = np.zeros(48, np.uint64)
        self._check(self._L.bn_pairing_batch(self._h, _ptr(p), _ptr(q), p.shape[0], _ptr(out)))
        return out

    def pairing_batch_many(self, p, q, offsets):
        """bn_pairing_batch_many: row j of the (m, 48) result is pairing_batch of the pairs
        offsets[j] <= i < offsets[j + 1].  offsets: m + 1 entries, non-decreasing from 0 to
        the number of pairs (ValueError otherwise)."""
        p, q = _arr(p, 12), _arr(q, 24)
        off = _offsets(offsets, _same_rows(p, q))
        m = off.shape[0] - 1
        out = np.zeros((m, 48), np.uint64)
        self._check(self._L.bn_pairing_batch_many(self._h, _ptr(p), _ptr(q), _ptr(off), m, _ptr(out)))
        return out

    def miller_loop_batch(self, q, p):
        q, p = _arr(q, 24), _arr(p, 12)
        _same_rows(q, p)
        out = np.zeros(48, np.uint64)
        self._check(self._L.bn_miller_loop_batch(self._h, _ptr(q), _ptr(p), q.shape[0], _ptr(out)))
        return out

    def miller_loop_many(self, p, q):
        p, q = _arr(p, 12), _arr(q, 24)
        _same_rows(p, q)
        out = np.zeros((p.shape[0], 48), np.uint64)
        self._check(self._L.bn_miller_loop_many(self._h, _ptr(p), _ptr(q), p.shape[0], _ptr(out)))
        return out

    def g2_precompute_many(self, q):
        """AffineG2::precompute of each (Jacobian) q: (n, 87, 24) uint64 -- per coefficient
        ell_0, ell_vw, ell_vv (mod.rs:566-577, 701-727)."""
        q = _arr(q, 24)
        out = np.zeros((q.shape[0], 87, 24), np.uint64)
        self._check(self._L.bn_g2_precompute_many(self._h, _ptr(q), q.shape[0], _ptr(out)))
        return out

    # ---- pairings against prepared G2 points (bn_g2_prepared)
    def g2_prepare(self, q):
        """bn_g2_prepare: a handle (int) holding the line coefficients of the rows of q on the
        device; release it with g2_prepared_destroy (substrate_bn.G2Prepared does)."""
        q = _arr(q, 24)
        h = ctypes.c_void_p()
        self._check(self._L.bn_g2_prepare(self._h, _ptr(q), q.shape[0], ctypes.byref(h)))
        return h.value

    def g2_prepare_dev(self, d_q, nq, stream=None):
        h = ctypes.c_void_p()
        self._check(self._L.bn_g2_prepare_dev(self._h, d_q, nq, ctypes.byref(h), stream))
        return h.value

    def g2_prepared_count(self, handle):
        return int(self._L.bn_g2_prepared_count(handle))

    def g2_prepared_destroy(self, handle):
        self._check(self._L.bn_g2_prepared_destroy(self._h, handle))

    def _prepared_many(self, fn, p, handle, idx):
        p = _arr(p, 12)
        n = p.shape[0]
        ix = _indices(idx, n, self.g2_prepared_count(handle))
        out = np.zeros((n, 48), np.uint64)
        self._check(fn(self._h, _ptr(p), handle, None if ix is None else _ptr(ix), n, _ptr(out)))
        return out

    def pairing_prepared_many(self, p, handle, idx=None):
        """bn_pairing_prepared_many: row i = pairing(p[i], Q[idx[i]]) for the handle's points Q;
        idx None passes a NULL index (every pair takes Q[0]).  Indices are checked here
        (ValueError) before the call."""
        return self._prepared_many(self._L.bn_pairing_prepared_many, p, handle, idx)

    def miller_loop_prepared_many(self, p, handle, idx=None):
        """bn_miller_loop_prepared_many: the Miller values of the same pairs."""
        return self._prepared_many(self._L.bn_miller_loop_prepared_many, p, handle, idx)

    def pairing_prepared_many_dev(self, d_p, handle, d_idx, n, d_out, stream=None):
        """bn_pairing_prepared_many_dev: device addresses (d_idx may be None); an index past the
        handle's points makes that row zero and dev_status() raise BN_ERR_INVALID_ARGUMENT."""
        self._check(self._L.bn_pairing_prepared_many_dev(self._h, d_p, handle, d_idx, n, d_out, stream))

    def pairing_batch_prepared_many(self, p, q, handle, qidx, offsets):
        """bn_pairing_batch_prepared_many: row j of the (m, 48) result is pairing_batch of the
        terms offsets[j] <= i < offsets[j + 1], term i pairing p[i] with the handle's point
        qidx[i], or with the next unused row of q where qidx[i] == QIDX_FRESH (q holds only
        those terms' points, in term order).  Indices, offsets, the row count of q and the
        64-term limit per product are checked here (ValueError) before the call; the empty
        call returns without one."""
        p = _arr(p, 12)
        n = p.shape[0]
        off = _offsets(offsets, n)
        _product_lengths(off)
        ix, nf = _term_indices(qidx, n, self.g2_prepared_count(handle))
        q = np.zeros((0, 24), np.uint64) if q is None else _arr(q, 24)
        if q.shape[0] != nf:
            raise ValueError("q has %d rows but %d terms are fresh" % (q.shape[0], nf))
        m = off.shape[0] - 1
        out = np.zeros((m, 48), np.uint64)
        if m == 0:
            return out
        self._check(self._L.bn_pairing_batch_prepared_many(self._h, _ptr(p) if n else None, _ptr(q) if nf else None,
                                                           handle, _ptr(ix), _ptr(off), m, _ptr(out)))
        return out

    def pairing_batch_prepared_many_dev(self, d_p, d_q, handle, qidx, offsets, d_out, stream=None):
        """bn_pairing_batch_prepared_many_dev: d_p, d_q (the fresh terms' points, compacted) and
        d_out are device addresses; qidx and offsets are HOST sequences, checked as in
        pairing_batch_prepared_many; the outcome is read with dev_status()."""
        off = _offsets(offsets)
        _product_lengths(off)
        ix, _ = _term_indices(qidx, int(off[-1]), self.g2_prepared_count(handle))
        if off.shape[0] == 1:
            return
        self._check(self._L.bn_pairing_batch_prepared_many_dev(self._h, d_p, d_q, handle, _ptr(ix), _ptr(off),
                                                               off.shape[0] - 1, d_out, stream))

    def final_exponentiation_many(self, f):
        f = _arr(f, 48)
        out = np.zeros_like(f)
        ok = np.zeros(f.shape[0], np.uint8)
        self._check(self._L.bn_final_exponentiation_many(self._h, _ptr(f), f.shape[0], _ptr(out), _ptr(ok)))
        return out, ok

    # ---- group path
    def g1_mul_many(self, p, k):
        p, k = _arr(p, 12), _arr(k, 4)
        _same_rows(p, k)
        out = np.zeros_like(p)
        self._check(self._L.bn_g1_mul_many(self._h, _ptr(p), _ptr(k), p.shape[0], _ptr(out)))
        return out

    def g2_mul_many(self, p, k):
        p, k = _arr(p, 24), _arr(k, 4)
        _same_rows(p, k)
        out = np.zeros_like(p)
        self._check(self._L.bn_g2_mul_many(self._h, _ptr(p), _ptr(k), p.shape[0], _ptr(out)))
        return out

    def g1_msm(self, p, k):
        """bn_g1_msm: the normalized image (12 words) of sum p[i] * k[i]; G1::zero() when
        the sum is zero or there are no terms."""
        p, k = _arr(p, 12), _arr(k, 4)
        n = _same_rows(p, k)
        out = np.zeros(12, np.uint64)
        self._check(self._L.bn_g1_msm(self._h, _ptr(p), _ptr(k), n, _ptr(out)))
        return out

    def g2_msm(self, p, k):
        """bn_g2_msm: the normalized image (24 words) of sum p[i] * k[i]; G2::zero() when
        the sum is zero or there are no terms."""
        p, k = _arr(p, 24), _arr(k, 4)
        n = _same_rows(p, k)
        out = np.zeros(24, np.uint64)
        self._check(self._L.bn_g2_msm(self._h, _ptr(p), _ptr(k), n, _ptr(out)))
        return out

    # ---- MSMs over prepared G1 bases (bn_g1_prepared)
    def g1_bases_prepare(self, bases, c=0):
        """bn_g1_bases_prepare: a handle (int) holding the window table of the rows of `bases`
        at width c (0: the default) on the device; release it with g1_prepared_destroy
        (substrate_bn.G1Prepared does)."""
        b = _arr(bases, 12)
        h = ctypes.c_void_p()
        self._check(self._L.bn_g1_bases_prepare(self._h, _ptr(b), b.shape[0], c, ctypes.byref(h)))
        return h.value

    def g1_bases_prepare_dev(self, d_bases, k, c=0, stream=None):
        h = ctypes.c_void_p()
        self._check(self._L.bn_g1_bases_prepare_dev(self._h, d_bases, k, c, ctypes.byref(h), stream))
        return h.value

    def g1_prepared_count(self, handle):
        return int(self._L.bn_g1_prepared_count(handle))

    def g1_prepared_window(self, handle):
        return int(self._L.bn_g1_prepared_window(handle))

    def g1_prepared_destroy(self, handle):
        self._check(self._L.bn_g1_prepared_destroy(self._h, handle))

    def g1_msm_prepared_many(self, handle, scalars, out_stride=1):
        """bn_g1_msm_prepared_many: scalars is an (m, k) matrix of Fr images -- (m, k, 4) words,
        or (m, 4) when the handle has one base -- and row j of the (m, 12) result is the
        normalized image of sum_b bases[b] * scalars[j, b].  With out_stride > 1 the result
        is the (m * out_stride, 12) strided buffer itself: row j * out_stride holds output j and
        the other rows stay zero.  A matrix whose width is not the handle's count and an
        out_stride below 1 raise ValueError before any native call."""
        k = self.g1_prepared_count(handle)
        s = np.ascontiguousarray(scalars, dtype=np.uint64)
        if out_stride < 1:
            raise ValueError("out_stride must be at least 1, not %d" % out_stride)
        if s.ndim == 3 and s.shape[1:] == (k, 4):
            m = s.shape[0]
        elif s.ndim == 2 and k == 1 and s.shape[1] == 4:
            m = s.shape[0]
        else:
            raise ValueError("scalars of shape %s are not rows of %d Fr images" % (s.shape, k))
        out = np.zeros((m * out_stride, 12), np.uint64)
        self._check(self._L.bn_g1_msm_prepared_many(self._h, handle, _ptr(s), m, _ptr(out), out_stride))
        return out

    def g1_msm_prepared_many_dev(self, handle, d_k, m, d_out, out_stride=1, stream=None):
        if out_stride < 1:
            raise ValueError("out_stride must be at least 1, not %d" % out_stride)
        self._check(self._L.bn_g1_msm_prepared_many_dev(self._h, handle, d_k, m, d_out, out_stride, stream))

    def set_msm_prepared_lanes(self, lanes):
        """Lanes per output of the prepared-bases lookup kernel: a power of two from 1 to 64;
        0: chosen from m and k."""
        self._check(self._L.bn_set_msm_prepared_lanes(self._h, lanes))

    # ---- many small MSMs over fresh bases (bn_g1_msm_many)
    def g1_msm_many(self, p, k, offsets, out_stride=1):
        """bn_g1_msm_many: row j of the (m, 12) result is the normalized image of the sum of
        p[i] * k[i] over offsets[j] <= i < offsets[j + 1] (G1::zero() for an empty segment or a
        zero sum).  With out_stride > 1 the result is the (m * out_stride, 12) strided buffer
        itself: row j * out_stride holds output j and the other rows stay zero.  Malformed
        offsets, offsets that do not end at the row count, p and k of different lengths and an
        out_stride below 1 raise ValueError before any native call."""
        p, k = _arr(p, 12), _arr(k, 4)
        n = _same_rows(p, k)
        if out_stride < 1:
            raise ValueError("out_stride must be at least 1, not %d" % out_stride)
        off = _offsets(offsets, n)
        m = off.shape[0] - 1
        out = np.zeros((m * out_stride, 12), np.uint64)
        if m == 0:
            return out
        self._check(self._L.bn_g1_msm_many(self._h, _ptr(p) if n else None, _ptr(k) if n else None, _ptr(off), m,
                                           _ptr(out), out_stride))
        return out

    def g1_msm_many_dev(self, d_p, d_k, offsets, d_out, out_stride=1, stream=None):
        """bn_g1_msm_many_dev: d_p, d_k and d_out are device addresses; offsets stays on the host
        and is checked as in g1_msm_many.  Nothing is reported: no outcome depends on the data."""
        if out_stride < 1:
            raise ValueError("out_stride must be at least 1, not %d" % out_stride)
        off = _offsets(offsets)
        self._check(self._L.bn_g1_msm_many_dev(self._h, d_p, d_k, _ptr(off), off.shape[0] - 1, d_out, out_stride,
                                               stream))

    def set_msm_many_window(self, c):
        """Window width of bn_g1_msm_many's packed path: 2 .. 8; 0: the default."""
        self._check(self._L.bn_set_msm_many_window(self._h, c))

    def set_msm_many_unit(self, terms):
        """Terms per unit (one lane's shared doublings): 1 .. 64; 0: chosen per launch set."""
        self._check(self._L.bn_set_msm_many_unit(self._h, terms))

    def set_msm_many_max(self, terms):
        """Segments of more terms run alone on g1_msm's path: at most 4096; 0: the default."""
        self._check(self._L.bn_set_msm_many_max(self._h, terms))

    def set_msm_many_chunk(self, terms):
        """The most terms of a launch set of the packed path; 0: the default."""
        self._check(self._L.bn_set_msm_many_chunk(self._h, terms))

    def g1_msm_many_reserve(self, terms, segments):
        self._check(self._L.bn_g1_msm_many_reserve(self._h, terms, segments))

    # ---- one large MSM over a fixed basis (bn_g1_basis)
    def g1_basis_prepare(self, bases, c=0):
        """bn_g1_basis_prepare: a handle (int) holding, for every row of `bases` and every
        window of width c (0: the default from the number of bases), the point 2^(c w) * base
        on the device; release it with g1_basis_destroy (substrate_bn.G1Basis does)."""
        b = _arr(bases, 12)
        h = ctypes.c_void_p()
        self._check(self._L.bn_g1_basis_prepare(self._h, _ptr(b), b.shape[0], c, ctypes.byref(h)))
        return h.value

    def g1_basis_prepare_dev(self, d_bases, nbases, c=0, stream=None):
        h = ctypes.c_void_p()
        self._check(self._L.bn_g1_basis_prepare_dev(self._h, d_bases, nbases, c, ctypes.byref(h), stream))
        return h.value

    def g1_basis_count(self, handle):
        return int(self._L.bn_g1_basis_count(handle))

    def g1_basis_window(self, handle):
        return int(self._L.bn_g1_basis_window(handle))

    def g1_basis_destroy(self, handle):
        self._check(self._L.bn_g1_basis_destroy(self._h, handle))

    def g1_msm_basis(self, handle, k):
        """bn_g1_msm_basis: the normalized image (12 words) of sum bases[i] * k[i] over the
        first len(k) bases of the handle; G1::zero() when the sum is zero or k is empty.  More
        scalars than the handle has bases raise ValueError before any native call."""
        k = _arr(k, 4)
        n = k.shape[0]
        if n > self.g1_basis_count(handle):
            raise ValueError("%d scalars for a basis of %d" % (n, self.g1_basis_count(handle)))
        out = np.zeros(12, np.uint64)
        self._check(self._L.bn_g1_msm_basis(self._h, handle, _ptr(k) if n else None, n, _ptr(out)))
        return out

    def g1_msm_basis_dev(self, handle, d_k, n, d_out, stream=None):
        """bn_g1_msm_basis_dev: d_k and d_out are device addresses; only enqueues."""
        self._check(self._L.bn_g1_msm_basis_dev(self._h, handle, d_k, n, d_out, stream))

    def g1_msm_basis_reserve(self, handle, n):
        self._check(self._L.bn_g1_msm_basis_reserve(self._h, handle, n))

    # ---- a batch of scalar vectors over a fixed basis (bn_g1_msm_basis_many)
    def g1_msm_basis_many(self, handle, scalars, n=None, out_stride=1):
        """bn_g1_msm_basis_many: scalars is an (m, k_stride, 4) array of Fr images; row j of the
        (m, 12) result is the normalized image of sum bases[i] * scalars[j, i] over the first n
        (default: k_stride) bases of the handle, G1::zero() for a zero sum or n == 0.  With
        out_stride > 1 the result is the (m * out_stride, 12) strided buffer itself: row
        j * out_stride holds output j and the other rows stay zero.  Scalars that are not such
        rows, an n above the row length or the handle's count and an out_stride below 1 raise
        ValueError before any native call."""
        s = np.ascontiguousarray(scalars, dtype=np.uint64)
        if s.ndim != 3 or s.shape[2] != 4:
            raise ValueError("scalars of shape %s are not rows of Fr images" % (s.shape,))
        m, k_stride = s.shape[0], s.shape[1]
        n = k_stride if n is None else n
        if n < 0 or n > k_stride:
            raise ValueError("n = %d outside rows of %d scalars" % (n, k_stride))
        if n > self.g1_basis_count(handle):
            raise ValueError("%d scalars for a basis of %d" % (n, self.g1_basis_count(handle)))
        if out_stride < 1:
            raise ValueError("out_stride must be at least 1, not %d" % out_stride)
        out = np.zeros((m * out_stride, 12), np.uint64)
        if m == 0:
            return out
        self._check(self._L.bn_g1_msm_basis_many(self._h, handle, _ptr(s) if n else None, k_stride, m, n, _ptr(out),
                                                 out_stride))
        return out

    def g1_msm_basis_many_dev(self, handle, d_k, k_stride, m, n, d_out, out_stride=1, stream=None):
        """bn_g1_msm_basis_many_dev: d_k and d_out are device addresses; only enqueues."""
        if out_stride < 1:
            raise ValueError("out_stride must be at least 1, not %d" % out_stride)
        if k_stride < n:
            raise ValueError("k_stride = %d below n = %d" % (k_stride, n))
        self._check(self._L.bn_g1_msm_basis_many_dev(self._h, handle, d_k, k_stride, m, n, d_out, out_stride, stream))

    def g1_msm_basis_many_reserve(self, handle, m, n):
        self._check(self._L.bn_g1_msm_basis_many_reserve(self._h, handle, m, n))

    def set_msm_basis_many_set(self, vectors):
        """Vectors per launch set of bn_g1_msm_basis_many: at most 2^26; 0: the default."""
        self._check(self._L.bn_set_msm_basis_many_set(self._h, vectors))

    # ---- the same over G2 (bn_g2_basis)
    def g2_basis_prepare(self, bases, c=0):
        """bn_g2_basis_prepare: a handle (int) holding, for every row of `bases` (24 words) and
        every window of width c (0: the default from the number of bases), the point
        2^(c w) * base on the device; release it with g2_basis_destroy (substrate_bn.G2Basis does)."""
        b = _arr(bases, 24)
        h = ctypes.c_void_p()
        self._check(self._L.bn_g2_basis_prepare(self._h, _ptr(b), b.shape[0], c, ctypes.byref(h)))
        return h.value

    def g2_basis_prepare_dev(self, d_bases, nbases, c=0, stream=None):
        h = ctypes.c_void_p()
        self._check(self._L.bn_g2_basis_prepare_dev(self._h, d_bases, nbases, c, ctypes.byref(h), stream))
        return h.value

    def g2_basis_count(self, handle):
        return int(self._L.bn_g2_basis_count(handle))

    def g2_basis_window(self, handle):
        return int(self._L.bn_g2_basis_window(handle))

    def g2_basis_destroy(self, handle):
        self._check(self._L.bn_g2_basis_destroy(self._h, handle))

    def g2_msm_basis(self, handle, k):
        """bn_g2_msm_basis: the normalized image (24 words) of sum bases[i] * k[i] over the
        first len(k) bases of the handle; G2::zero() when the sum is zero or k is empty.  More
        scalars than the handle has bases raise ValueError before any native call."""
        k = _arr(k, 4)
        n = k.shape[0]
        if n > self.g2_basis_count(handle):
            raise ValueError("%d scalars for a basis of %d" % (n, self.g2_basis_count(handle)))
        out = np.zeros(24, np.uint64)
        self._check(self._L.bn_g2_msm_basis(self._h, handle, _ptr(k) if n else None, n, _ptr(out)))
        return out

    def g2_msm_basis_dev(self, handle, d_k, n, d_out, stream=None):
        """bn_g2_msm_basis_dev: d_k and d_out are device addresses; only enqueues."""
        self._check(self._L.bn_g2_msm_basis_dev(self._h, handle, d_k, n, d_out, stream))

    def g2_msm_basis_reserve(self, handle, n):
        self._check(self._L.bn_g2_msm_basis_reserve(self._h, handle, n))

    def fq12_op_many(self, op, a, b=None):
        a = _arr(a, 48)
        bb = _arr(b, 48) if b is not None else None
        if op == "mul":
            if bb is None:
                raise ValueError("fq12 mul needs two operands")
            _same_rows(a, bb)
        out = np.zeros_like(a)
        self._check(self._L.bn_fq12_op_many(self._h, FQ12_OPS[op], _ptr(a), _ptr(bb) if bb is not None else None,
                                            a.shape[0], _ptr(out)))
        return out

    # ---- device-pointer variants (ints: device addresses, e.g. torch tensor.data_ptr())
    def pairing_many_dev(self, d_p, d_q, n, d_out, stream=None):
        self._check(self._L.bn_pairing_many_dev(self._h, d_p, d_q, n, d_out, stream))

    def g1_mul_many_dev(self, d_p, d_k, n, d_out, stream=None):
        self._check(self._L.bn_g1_mul_many_dev(self._h, d_p, d_k, n, d_out, stream))

    def g2_mul_many_dev(self, d_p, d_k, n, d_out, stream=None):
        self._check(self._L.bn_g2_mul_many_dev(self._h, d_p, d_k, n, d_out, stream))

    def g1_msm_dev(self, d_p, d_k, n, d_out, stream=None):
        self._check(self._L.bn_g1_msm_dev(self._h, d_p, d_k, n, d_out, stream))

    def g2_msm_dev(self, d_p, d_k, n, d_out, stream=None):
        self._check(self._L.bn_g2_msm_dev(self._h, d_p, d_k, n, d_out, stream))

    def set_msm_window(self, c):
        """Window width in bits of the MSM bucket path of both groups (2 .. 16); 0: chosen
        from n by the group's own table."""
        self._check(self._L.bn_set_msm_window(self._h, c))

    def set_msm_min(self, n):
        """MSM batches below n terms take the small path; 0: always the bucket path."""
        self._check(self._L.bn_set_msm_min(self._h, n))

    def set_msm_run_max(self, entries):
        """The run cap of the MSM bucket path of both groups: a bucket with more entries is
        summed in chunks of that many and a fold tree.  0: the default rule; 1 .. 65536: that
        cap; MSM_RUN_UNSPLIT: never split.  No value changes a result."""
        self._check(self._L.bn_set_msm_run_max(self._h, entries))

    def msm_reserve(self, n):
        self._check(self._L.bn_msm_reserve(self._h, n))

    def g2_msm_reserve(self, n):
        self._check(self._L.bn_g2_msm_reserve(self._h, n))

    def pairing_batch_dev(self, d_p, d_q, n, d_out, d_status=None, stream=None):
        self._check(self._L.bn_pairing_batch_dev(self._h, d_p, d_q, n, d_out, d_status, stream))

    def miller_loop_batch_dev(self, d_q, d_p, n, d_out, d_status=None, stream=None):
        self._check(self._L.bn_miller_loop_batch_dev(self._h, d_q, d_p, n, d_out, d_status, stream))

    def pairing_batch_many_dev(self, d_p, d_q, offsets, d_out, stream=None):
        """bn_pairing_batch_many_dev: d_p, d_q, d_out are device addresses, offsets a HOST
        sequence of m + 1 entries (checked as in pairing_batch_many); the outcome is read
        with dev_status()."""
        off = _offsets(offsets)
        self._check(self._L.bn_pairing_batch_many_dev(self._h, d_p, d_q, _ptr(off), off.shape[0] - 1, d_out, stream))

    def set_products_min(self, m):
        """pairing_batch_many calls with fewer than m products of at most 64 terms run each
        product on the single-product path; 0: always the packed kernel."""
        self._check(self._L.bn_set_products_min(self._h, m))

    def set_products_chunk(self, terms):
        """Terms per launch set of the packed path; 0: the default (2^18), which is also the
        largest value accepted."""
        self._check(self._L.bn_set_products_chunk(self._h, terms))

    def set_products_wide_max(self, terms):
        """Product calls (pairing_batch_many, pairing_batch_prepared_many) of at most `terms`
        terms take the wide path: the latency kernel's Miller value per term, a 16-lane group
        per product.  0 turns it off.  A negative or non-integer value raises ValueError."""
        if isinstance(terms, bool) or not isinstance(terms, (int, np.integer)):
            raise ValueError("terms must be an integer")
        if terms < 0 or terms >= 1 << 64:
            raise ValueError("terms must be within 0 .. 2^64 - 1")
        self._check(self._L.bn_set_products_wide_max(self._h, int(terms)))

    def products_routes(self):
        """(wide, packed, alone): the products the product calls planned on each path since
        the last read, which clears the counts."""
        counts = np.zeros(3, np.uintp)
        self._check(self._L.bn_get_products_routes(self._h, _ptr(counts)))
        return tuple(int(v) for v in counts)

    def set_fe_wide_max(self, n):
        """Batches of at most n elements use the 16-lane final exponentiation (latency path)."""
        self._check(self._L.bn_set_fe_wide_max(self._h, n))

    def set_fq12_op_unit(self, unit):
        """fq12_op_many's step machine: 0 = the final-exponentiation unit's, 1 = the throughput kernel's unit's."""
        self._check(self._L.bn_set_fq12_op_unit(self._h, unit))

    def set_latency_max(self, n):
        """Latency-path batches of at most n pairs run the one-launch k_pairing_latency."""
        self._check(self._L.bn_set_latency_max(self._h, n))

    def set_phase_timing(self, enable=True):
        self._check(self._L.bn_set_phase_timing(self._h, 1 if enable else 0))

    def phase_times(self):
        """(ms per phase [prepare, miller, final_exp, fe_out], launch sets) since the last read."""
        ms = np.zeros(4, np.float32)
        cnt = np.zeros(1, np.int32)
        self._check(self._L.bn_get_phase_times(self._h, _ptr(ms), _ptr(cnt)))
        return ms.astype(float), int(cnt[0])

    # ---- encodings / validation / square roots / decompression / Gt::pow
    def _bytes_in(self, b, width):
        b = np.ascontiguousarray(b, dtype=np.uint8)
        if b.size % width:
            raise ValueError("byte buffer of %d is not a multiple of %d" % (b.size, width))
        return b.reshape(-1, width)

    def fq_from_slice_many(self, be32):
        b = self._bytes_in(be32, 32)
        out = np.zeros((b.shape[0], 4), np.uint64)
        st = np.zeros(b.shape[0], np.uint8)
        self._check(self._L.bn_fq_from_slice_many(self._h, _ptr(b), b.shape[0], _ptr(out), _ptr(st)))
        return out, st

    def fq_to_big_endian_many(self, a):
        a = _arr(a, 4)
        out = np.zeros((a.shape[0], 32), np.uint8)
        self._check(self._L.bn_fq_to_big_endian_many(self._h, _ptr(a), a.shape[0], _ptr(out)))
        return out

    def fq2_from_slice_many(self, be64):
        b = self._bytes_in(be64, 64)
        out = np.zeros((b.shape[0], 8), np.uint64)
        st = np.zeros(b.shape[0], np.uint8)
        self._check(self._L.bn_fq2_from_slice_many(self._h, _ptr(b), b.shape[0], _ptr(out), _ptr(st)))
        return out, st

    def fr_from_slice_many(self, be32):
        b = self._bytes_in(be32, 32)
        out = np.zeros((b.shape[0], 4), np.uint64)
        self._check(self._L.bn_fr_from_slice_many(self._h, _ptr(b), b.shape[0], _ptr(out)))
        return out

    def fr_to_big_endian_many(self, a):
        a = _arr(a, 4)
        out = np.zeros((a.shape[0], 32), np.uint8)
        self._check(self._L.bn_fr_to_big_endian_many(self._h, _ptr(a), a.shape[0], _ptr(out)))
        return out

    def fq_sqrt_many(self, a):
        a = _arr(a, 4)
        out = np.zeros_like(a)
        ok = np.zeros(a.shape[0], np.uint8)
        self._check(self._L.bn_fq_sqrt_many(self._h, _ptr(a), a.shape[0], _ptr(out), _ptr(ok)))
        return out, ok

    def fq2_sqrt_many(self, a):
        a = _arr(a, 8)
        out = np.zeros_like(a)
        ok = np.zeros(a.shape[0], np.uint8)
        self._check(self._L.bn_fq2_sqrt_many(self._h, _ptr(a), a.shape[0], _ptr(out), _ptr(ok)))
        return out, ok

    def g1_affine_new_many(self, x, y):
        x, y = _arr(x, 4), _arr(y, 4)
        _same_rows(x, y)
        out = np.zeros((x.shape[0], 12), np.uint64)
        st = np.zeros(x.shape[0], np.uint8)
        self._check(self._L.bn_g1_affine_new_many(self._h, _ptr(x), _ptr(y), x.shape[0], _ptr(out), _ptr(st)))
        return out, st

    def g2_affine_new_many(self, x, y):
        x, y = _arr(x, 8), _arr(y, 8)
        _same_rows(x, y)
        out = np.zeros((x.shape[0], 24), np.uint64)
        st = np.zeros(x.shape[0], np.uint8)
        self._check(self._L.bn_g2_affine_new_many(self._h, _ptr(x), _ptr(y), x.shape[0], _ptr(out), _ptr(st)))
        return out, st

    def g1_from_compressed_many(self, b33):
        b = self._bytes_in(b33, 33)
        out = np.zeros((b.shape[0], 12), np.uint64)
        st = np.zeros(b.shape[0], np.uint8)
        self._check(self._L.bn_g1_from_compressed_many(self._h, _ptr(b), b.shape[0], _ptr(out), _ptr(st)))
        return out, st

    def g2_from_compressed_many(self, b65):
        b = self._bytes_in(b65, 65)
        out = np.zeros((b.shape[0], 24), np.uint64)
        st = np.zeros(b.shape[0], np.uint8)
        self._check(self._L.bn_g2_from_compressed_many(self._h, _ptr(b), b.shape[0], _ptr(out), _ptr(st)))
        return out, st

    def gt_pow_many(self, a, k):
        a, k = _arr(a, 48), _arr(k, 4)
        _same_rows(a, k)
        out = np.zeros_like(a)
        self._check(self._L.bn_gt_pow_many(self._h, _ptr(a), _ptr(k), a.shape[0], _ptr(out)))
        return out

    def g2_affine_new_many_dev(self, d_x, d_y, n, d_out, d_st, stream=None):
        self._check(self._L.bn_g2_affine_new_many_dev(self._h, d_x, d_y, n, d_out, d_st, stream))

    def g1_from_compressed_many_dev(self, d_b, n, d_out, d_st, stream=None):
        self._check(self._L.bn_g1_from_compressed_many_dev(self._h, d_b, n, d_out, d_st, stream))

    def g2_from_compressed_many_dev(self, d_b, n, d_out, d_st, stream=None):
        self._check(self._L.bn_g2_from_compressed_many_dev(self._h, d_b, n, d_out, d_st, stream))

    def gt_pow_many_dev(self, d_a, d_k, n, d_out, stream=None):
        self._check(self._L.bn_gt_pow_many_dev(self._h, d_a, d_k, n, d_out, stream))

    def reserve(self, n):
        self._check(self._L.bn_reserve(self._h, n))


def workspace_bytes(n):
    return load().bn_workspace_bytes(n)


def g1_prepared_table_bytes(k, c=0):
    """bn_g1_prepared_table_bytes: device bytes of the table of k bases at width c (0: the
    default); 0 for arguments the prepare call refuses.  Host arithmetic, no device."""
    return load().bn_g1_prepared_table_bytes(k, c)


def g1_basis_table_bytes(nbases, c=0):
    """bn_g1_basis_table_bytes: device bytes of the fixed-basis table of nbases bases at width
    c (0: the default); 0 for arguments the prepare call refuses.  Host arithmetic, no device."""
    return load().bn_g1_basis_table_bytes(nbases, c)


def g2_basis_table_bytes(nbases, c=0):
    """bn_g2_basis_table_bytes: the same for a G2 basis (128 bytes per entry)."""
    return load().bn_g2_basis_table_bytes(nbases, c)
