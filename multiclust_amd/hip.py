"""ctypes view of include/multiclust_hip.h (libmulticlust_hip.so)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PROF_KINDS = 4
ABI_VERSION = 2          # MCHIP_ABI_VERSION of include/multiclust_hip.h these bindings were written against
STATUS = {0: "OK", 1: "INVALID", 2: "NO_DEVICE", 3: "HIP", 4: "ALLOC", 5: "STATE", 6: "UNSUPPORTED"}


class HipError(RuntimeError):
    pass


class RunState(C.Structure):
    """mchip_run_state (include/multiclust_hip.h)"""
    _fields_ = [("logL", C.c_double), ("bad_loglik", C.c_double), ("abs_error", C.c_double), ("rel_error", C.c_double),
                ("n_iter", C.c_int), ("max_iter", C.c_int), ("stopped", C.c_int), ("converged", C.c_int),
                ("iter_stop", C.c_int), ("fatal", C.c_int)]


class PlanQuery(C.Structure):
    """mchip_plan_query (include/multiclust_hip.h)"""
    _fields_ = [("K", C.c_int), ("I", C.c_int), ("L", C.c_int), ("T", C.c_int), ("ploidy", C.c_int),
                ("min_alleles", C.c_int), ("max_alleles", C.c_int), ("has_missing", C.c_int),
                ("admixture", C.c_int), ("eta_constrained", C.c_int), ("do_projection", C.c_int),
                ("p_lb", C.c_double), ("n_cu", C.c_int), ("accel_cycle", C.c_int)]


def lib_path():
    # MCHIP_LIB_PATH: an experimental build of the library (scripts/diag/*_exp.sh); the product path is the in-tree one
    return os.environ.get("MCHIP_LIB_PATH") or os.path.join(_HERE, "lib", "libmulticlust_hip.so")


_lib = None


def load():
    """Load the HIP library. Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise HipError("%s is missing: run `make` (or __graft_entry__.build()); there is no CPU fallback" % path)
    lib = C.CDLL(path)
    vp, dp, i32 = C.c_void_p, C.POINTER(C.c_double), C.c_int
    ip = C.POINTER(C.c_int)
    sig = {
        "mchip_abi_version": ([], i32),
        "mchip_device_count": ([ip], i32),
        "mchip_create": ([C.POINTER(vp), i32], i32),
        "mchip_destroy": ([vp], i32),
        "mchip_last_error": ([vp], C.c_char_p),
        "mchip_synchronize": ([vp], i32),
        "mchip_set_genotypes": ([vp, i32, i32, i32, vp, vp], i32),
        "mchip_set_genotypes_bed": ([vp, i32, i32, vp, C.c_size_t, vp], i32),
        "mchip_bed_ld_band": ([vp, i32, i32, vp, C.c_size_t, i32, i32, i32, vp], i32),
        "mchip_bed_king": ([vp, i32, i32, vp, C.c_size_t, i32, i32, vp, vp], i32),
        "mchip_bed_qc": ([vp, i32, i32, vp, C.c_size_t, vp, vp, vp, vp], i32),
        "mchip_bed_pca_apply": ([vp, i32, i32, vp, C.c_size_t, i32, vp, vp, vp, vp, vp, vp], i32),
        "mchip_bed_pca": ([vp, i32, i32, vp, C.c_size_t, i32, i32, i32, C.c_double, vp, vp, vp, vp, vp, vp], i32),
        "mchip_set_model": ([vp, i32, i32, i32, i32, C.c_double, C.c_double, i32], i32),
        "mchip_set_p": ([vp, i32, vp], i32),
        "mchip_get_p": ([vp, i32, vp], i32),
        "mchip_set_q": ([vp, i32, vp], i32),
        "mchip_get_q": ([vp, i32, vp], i32),
        "mchip_q_length": ([vp, ip], i32),
        "mchip_p_length": ([vp, ip], i32),
        "mchip_em_step": ([vp, i32, i32, dp], i32),
        "mchip_last_loglik": ([vp, dp], i32),
        "mchip_em_run": ([vp, i32, i32, vp], i32),
        "mchip_e_step": ([vp, i32, dp], i32),
        "mchip_loglik": ([vp, i32, dp], i32),
        "mchip_loglik_prefetch": ([vp, i32, dp], i32),
        "mchip_accel_run": ([vp, i32, i32, i32, vp], i32),
        "mchip_mstep_from_partition": ([vp, vp, i32], i32),
        "mchip_mstep_from_rand_partition": ([vp, vp, i32], i32),
        "mchip_get_genotypes": ([vp, vp], i32),
        "mchip_data_counts": ([vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)], i32),
        "mchip_empty_individuals": ([vp, C.POINTER(C.c_int)], i32),
        "mchip_copy_genotypes": ([vp, vp], i32),
        "mchip_simulate_genotypes": ([vp, i32, i32, i32, vp, vp, i32, i32, vp, vp], i32),
        "mchip_simulate_genotypes_mixture": ([vp, i32, i32, i32, vp, vp, i32, vp, vp], i32),
        "mchip_init_from_individual_centers": ([vp, vp, i32, vp], i32),
        "mchip_set_init_genotypes": ([vp, vp], i32),
        "mchip_get_expected_counts": ([vp, vp], i32),
        "mchip_init_from_allele_centers": ([vp, vp, vp, vp, C.c_uint64, i32], i32),
        "mchip_copy_slot": ([vp, i32, i32], i32),
        "mchip_secant": ([vp, i32, i32, i32, i32], i32),
        "mchip_set_secant": ([vp, i32, i32, vp, vp], i32),
        "mchip_get_secant": ([vp, i32, i32, vp, vp], i32),
        "mchip_step_dots": ([vp, i32, dp], i32),
        "mchip_secant_dots": ([vp, i32, i32, dp], i32),
        "mchip_accel_update": ([vp, i32, i32, i32, C.c_double, i32], i32),
        "mchip_multisecant_update": ([vp, i32, i32, i32, i32, ip, dp, dp], i32),
        "mchip_profile_begin": ([vp], i32),
        "mchip_profile_end": ([vp, dp, dp, ip], i32),
        "mchip_device_info": ([vp, C.c_char_p, i32, ip, dp], i32),
        "mchip_comm_create": ([C.POINTER(vp), i32, ip], i32),
        "mchip_comm_all_reduce": ([vp, C.POINTER(dp), i32, i32], i32),
        "mchip_comm_destroy": ([vp], i32),
        "mchip_comm_last_error": ([vp], C.c_char_p),
        "mchip_comm_info": ([vp, ip, ip, C.POINTER(C.c_ulonglong)], i32),
        "mchip_progress_report": ([C.c_char_p, i32, C.POINTER(C.c_ulonglong)], i32),
        "mchip_progress_note": ([C.c_char_p], i32),
        "mchip_cv_draw_folds": ([vp, vp, i32], i32),
        "mchip_cv_set_folds": ([vp, vp, i32], i32),
        "mchip_cv_get_folds": ([vp, vp], i32),
        "mchip_cv_hold_out": ([vp, i32], i32),
        "mchip_cv_heldout_loglik": ([vp, i32, C.c_double, dp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)], i32),
        "mchip_resample_loci": ([vp, vp, i32], i32),
        "mchip_fit_q_rows": ([vp, i32, vp, i32, i32, i32, C.c_double, C.c_double, vp, vp, vp, vp], i32),
        "mchip_impute_missing": ([vp, i32, vp, vp, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), dp], i32),
        "mchip_divergence": ([vp, i32, vp, vp, vp, vp, vp, dp, dp, ip], i32),
        "mchip_residual_products": ([vp, i32, vp, vp], i32),
        "mchip_kinship_products": ([vp, i32, vp, vp], i32),
        "mchip_describe_plan": ([C.POINTER(PlanQuery), C.c_char_p, i32], i32),
    }
    for name, (args, res) in sig.items():
        if os.environ.get("MCHIP_ALLOW_PARTIAL_ABI") == "1" and not hasattr(lib, name):
            continue                   # diagnostics only (scripts/diag/bits.sh: an older build under comparison); MCHIP_LIB_PATH alone
        fn = getattr(lib, name)        # keeps the strict check: AttributeError here = the library does not export its own header
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib


ABI_SYMBOLS = [
    "mchip_abi_version", "mchip_device_count", "mchip_create", "mchip_destroy", "mchip_last_error",
    "mchip_synchronize", "mchip_set_genotypes", "mchip_set_model", "mchip_set_p", "mchip_get_p", "mchip_set_q",
    "mchip_get_q", "mchip_q_length", "mchip_p_length", "mchip_em_step", "mchip_em_run", "mchip_accel_run", "mchip_last_loglik", "mchip_e_step",
    "mchip_loglik", "mchip_loglik_prefetch", "mchip_mstep_from_partition", "mchip_mstep_from_rand_partition",
    "mchip_get_genotypes", "mchip_data_counts", "mchip_empty_individuals", "mchip_copy_genotypes", "mchip_simulate_genotypes", "mchip_set_init_genotypes",
    "mchip_get_expected_counts", "mchip_init_from_allele_centers", "mchip_copy_slot", "mchip_secant", "mchip_set_secant", "mchip_get_secant", "mchip_step_dots",
    "mchip_secant_dots", "mchip_accel_update", "mchip_multisecant_update", "mchip_profile_begin",
    "mchip_profile_end", "mchip_device_info", "mchip_comm_create", "mchip_comm_all_reduce", "mchip_comm_destroy",
    "mchip_comm_last_error", "mchip_comm_info", "mchip_progress_report", "mchip_progress_note",
    "mchip_simulate_genotypes_mixture", "mchip_init_from_individual_centers", "mchip_set_genotypes_bed",
    "mchip_cv_draw_folds", "mchip_cv_set_folds", "mchip_cv_get_folds", "mchip_cv_hold_out", "mchip_cv_heldout_loglik",
    "mchip_resample_loci", "mchip_fit_q_rows", "mchip_impute_missing", "mchip_divergence",
    "mchip_residual_products", "mchip_kinship_products", "mchip_describe_plan", "mchip_bed_ld_band", "mchip_bed_king", "mchip_bed_qc",
    "mchip_bed_pca_apply", "mchip_bed_pca",
]


def describe_plan(**query):
    """mchip_describe_plan: (status, kernel names, {key: value}) of the library's kernel selection; needs no device"""
    buf = C.create_string_buffer(4096)
    rc = load().mchip_describe_plan(C.byref(PlanQuery(**query)), buf, len(buf))
    lines = buf.value.decode().split() if rc == 0 else []
    return rc, {x for x in lines if "=" not in x}, {x.split("=")[0]: int(x.split("=")[1]) for x in lines if "=" in x}


class Context:
    """One HIP context = one stream + device buffers for (device, data set, K)."""

    def __init__(self, device=0):
        self.lib = load()
        self.h = C.c_void_p()
        rc = self.lib.mchip_create(C.byref(self.h), device)
        if rc:
            raise HipError("mchip_create failed: %s (no GPU => no product path; nothing falls back to the CPU)" % STATUS.get(rc, rc))
        self.I = self.L = self.ploidy = self.T = self.K = 0
        self.indiv_q = True
        self._ua = self._rs_ua = None   # allele lists of the data set held and of the base of its selections (resample_loci)

    def _chk(self, rc):
        if rc:
            raise HipError("%s: %s" % (STATUS.get(rc, rc), self.lib.mchip_last_error(self.h).decode()))

    def close(self):
        if self.h:
            self.lib.mchip_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_genotypes(self, ua, geno):
        geno = np.ascontiguousarray(geno, dtype=np.uint8)
        ua = np.ascontiguousarray(ua, dtype=np.int32)
        I, L, p = geno.shape
        self._chk(self.lib.mchip_set_genotypes(self.h, I, L, p, ua.ctypes.data, geno.ctypes.data))
        self.I, self.L, self.ploidy, self.T = I, L, p, int(ua.sum())
        self._ua, self._rs_ua = ua.copy(), None

    def set_genotypes_bed(self, I, bed, record_bytes=None):
        """PLINK 1 packed records [L][record_bytes] (the .bed file behind its three header bytes; record_bytes defaults to the
        row length, at least ceil(I/4)), unpacked on the device (include/multiclust_hip.h); drops the model.  Returns the L
        allele counts the data set was installed with."""
        bed = np.ascontiguousarray(bed, dtype=np.uint8)
        assert bed.ndim == 2
        L = bed.shape[0]
        rb = bed.shape[1] if record_bytes is None else record_bytes
        assert rb == bed.shape[1] and rb >= (I + 3) // 4
        ua = np.empty(L, dtype=np.int32)
        self._chk(self.lib.mchip_set_genotypes_bed(self.h, I, L, bed.ctypes.data, rb, ua.ctypes.data))
        self.I, self.L, self.ploidy, self.T = I, L, 2, int(ua.sum())
        self._ua, self._rs_ua = ua.copy(), None
        return ua

    def bed_ld_band(self, I, bed, l0=0, n_first=None, window=50, record_bytes=None, L=None):
        """mchip_bed_ld_band: r2[n_first][window] of the variants l0 ... l0 + n_first - 1 of the packed records [L][record_bytes]
        with their `window` successors (include/multiclust_hip.h has the definition); NaN behind the last variant and where a
        variance is 0.  Installs nothing and changes nothing of the context."""
        bed = np.ascontiguousarray(bed, dtype=np.uint8)
        assert bed.ndim == 2
        L = bed.shape[0] if L is None else L
        rb = bed.shape[1] if record_bytes is None else record_bytes
        n_first = L - l0 if n_first is None else n_first
        out = np.empty((max(n_first, 0), max(window, 0)), dtype=np.float64)
        self._chk(self.lib.mchip_bed_ld_band(self.h, I, L, bed.ctypes.data, rb, l0, n_first, window, out.ctypes.data))
        return out

    def bed_king(self, I, bed, i0=0, n_rows=None, counts=True, record_bytes=None, L=None):
        """mchip_bed_king: (phi [n_rows][I], counts [n_rows][I][4] or None) of the individuals i0 ... i0 + n_rows - 1 against all I
        of the packed records [L][record_bytes]: the KING-robust kinship and the counts n, hh, op, h_ij it is formed from
        (include/multiclust_hip.h has the definition); NaN where min(h_ij, h_ji) = 0: either of the two has no heterozygous call at a
        variant where the other is typed.  Installs nothing and changes nothing of the context."""
        bed = np.ascontiguousarray(bed, dtype=np.uint8)
        assert bed.ndim == 2
        L = bed.shape[0] if L is None else L
        rb = bed.shape[1] if record_bytes is None else record_bytes
        n_rows = I - i0 if n_rows is None else n_rows
        phi = np.empty((max(n_rows, 0), max(I, 0)), dtype=np.float64)
        cnt = np.empty((max(n_rows, 0), max(I, 0), 4), dtype=np.uint32) if counts else None
        self._chk(self.lib.mchip_bed_king(self.h, I, L, bed.ctypes.data, rb, i0, n_rows, phi.ctypes.data,
                                          cnt.ctypes.data if counts else None))
        return phi, cnt

    def bed_qc(self, I, bed, ind_keep=None, ind=True, var=True, hwe=True, record_bytes=None, L=None):
        """mchip_bed_qc: (ind_counts [I][4], var_counts [L][4], hwe_p [L]) of the packed records [L][record_bytes], None for an
        array that was not asked for: the four genotype counts of every individual over all variants, of every variant over the
        individuals with ind_keep != 0 (None: all), and the Hardy-Weinberg exact test of the latter (include/multiclust_hip.h has
        the definition).  Installs nothing and changes nothing of the context."""
        bed = np.ascontiguousarray(bed, dtype=np.uint8)
        assert bed.ndim == 2
        L = bed.shape[0] if L is None else L
        rb = bed.shape[1] if record_bytes is None else record_bytes
        keep = None if ind_keep is None else np.ascontiguousarray(ind_keep, dtype=np.uint8)
        assert keep is None or keep.shape == (I,)
        ic = np.empty((max(I, 0), 4), dtype=np.uint32) if ind else None
        vc = np.empty((max(L, 0), 4), dtype=np.uint32) if var else None
        hp = np.empty(max(L, 0), dtype=np.float64) if hwe else None
        self._chk(self.lib.mchip_bed_qc(self.h, I, L, bed.ctypes.data, rb, None if keep is None else keep.ctypes.data,
                                        None if ic is None else ic.ctypes.data, None if vc is None else vc.ctypes.data,
                                        None if hp is None else hp.ctypes.data))
        return ic, vc, hp

    def bed_pca_apply(self, I, bed, x, w=True, scale=True, record_bytes=None, L=None):
        """mchip_bed_pca_apply: (y [I][n_vec], w [L][n_vec] or None, scale [L][2] or None, L', trace) of the packed records
        [L][record_bytes] and x [I][n_vec]: Y = Z (Z^T X) / L' with Z the mean-imputed standardised genotypes, W = Z^T X, scale = (mu, inv)
        of every variant (include/multiclust_hip.h has the definition).  Installs nothing and changes nothing of the context."""
        bed = np.ascontiguousarray(bed, dtype=np.uint8)
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert bed.ndim == 2 and x.ndim == 2 and x.shape[0] == I
        L = bed.shape[0] if L is None else L
        rb = bed.shape[1] if record_bytes is None else record_bytes
        n_vec = x.shape[1]
        y = np.empty((I, n_vec), dtype=np.float64)
        wo = np.empty((L, n_vec), dtype=np.float64) if w else None
        sc = np.empty((L, 2), dtype=np.float64) if scale else None
        n_used, trace = C.c_int(), C.c_double()
        self._chk(self.lib.mchip_bed_pca_apply(self.h, I, L, bed.ctypes.data, rb, n_vec, x.ctypes.data, y.ctypes.data,
                                               wo.ctypes.data if w else None, sc.ctypes.data if scale else None,
                                               C.byref(n_used), C.byref(trace)))
        return y, wo, sc, n_used.value, trace.value

    def bed_pca(self, I, bed, n_pc, n_extra=10, max_iter=200, tol=1e-6, record_bytes=None, L=None):
        """mchip_bed_pca: dict(eigenvalues [n_pc], eigenvectors [I][n_pc], residuals [n_pc], trace, n_used, n_iter) of the packed
        records [L][record_bytes]: the leading eigenpairs of G = Z Z^T / L' by block subspace iteration
        (include/multiclust_hip.h, csrc/mchip_pca_algebra.h).  Installs nothing and changes nothing of the context."""
        bed = np.ascontiguousarray(bed, dtype=np.uint8)
        assert bed.ndim == 2
        L = bed.shape[0] if L is None else L
        rb = bed.shape[1] if record_bytes is None else record_bytes
        val, vec, res = np.empty(n_pc), np.empty((I, n_pc)), np.empty(n_pc)
        trace, n_used, n_iter = C.c_double(), C.c_int(), C.c_int()
        self._chk(self.lib.mchip_bed_pca(self.h, I, L, bed.ctypes.data, rb, n_pc, n_extra, max_iter, tol, val.ctypes.data,
                                         vec.ctypes.data, res.ctypes.data, C.byref(trace), C.byref(n_used), C.byref(n_iter)))
        return dict(eigenvalues=val, eigenvectors=vec, residuals=res, trace=trace.value, n_used=n_used.value, n_iter=n_iter.value)

    def data_counts(self):
        """(cells with n_ic > 0, non-missing allele copies) of the data set held, counted on the device"""
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.mchip_data_counts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def copy_genotypes(self, src):
        """take the data set another context (same device) holds"""
        self._chk(self.lib.mchip_copy_genotypes(self.h, src.h))
        self.I, self.L, self.ploidy, self.T = src.I, src.L, src.ploidy, src.T
        self._ua, self._rs_ua = src._ua, None

    def get_genotypes(self):
        g = np.empty((self.I, self.L, self.ploidy), dtype=np.uint8)
        self._chk(self.lib.mchip_get_genotypes(self.h, g.ctypes.data))
        return g

    def empty_individuals(self):
        """(how many individuals of the data set held have no observed copy, the first one's index or -1)"""
        first = C.c_int(-1)
        n = self.lib.mchip_empty_individuals(self.h, C.byref(first))
        return n, first.value

    # ---- K-fold cross-validation (include/multiclust_hip.h, mchip_cv_*) ----
    def cv_draw_folds(self, window, n_folds):
        """fold of genotype (i, l) = rand() % n_folds from the stream `window` describes; consumes I*L draws"""
        w = np.ascontiguousarray(window, dtype=np.uint32)
        assert w.size == 31
        self._chk(self.lib.mchip_cv_draw_folds(self.h, w.ctypes.data, n_folds))

    def cv_set_folds(self, folds, n_folds):
        f = np.ascontiguousarray(folds, dtype=np.uint8)
        assert f.size == self.I * self.L
        self._chk(self.lib.mchip_cv_set_folds(self.h, f.ctypes.data, n_folds))

    def cv_get_folds(self):
        f = np.empty((self.I, self.L), dtype=np.uint8)
        self._chk(self.lib.mchip_cv_get_folds(self.h, f.ctypes.data))
        return f

    def cv_hold_out(self, fold):
        """install the data set with fold `fold` missing (-1: the full data set again); keeps the model"""
        self._chk(self.lib.mchip_cv_hold_out(self.h, fold))

    def cv_heldout_loglik(self, slot, floor):
        """(sum of log max(t, floor) over the observed copies of the fold held out, their number, how many were floored)"""
        s, n, nf = C.c_double(), C.c_uint64(), C.c_uint64()
        self._chk(self.lib.mchip_cv_heldout_loglik(self.h, slot, floor, C.byref(s), C.byref(n), C.byref(nf)))
        return s.value, n.value, nf.value

    def fit_q_rows(self, slot, rows, max_iter, abs_error=0.0, rel_error=0.0, from_slot=False, out=None):
        """mchip_fit_q_rows: the mixing proportions of the listed individuals fitted with P of `slot` held fixed, each row to its
        own convergence (include/multiclust_hip.h): (q [n][K], logL [n], iterations [n] int32, converged [n] uint8).  out: the four
        arrays to fill instead of new ones."""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        assert r.ndim == 1
        n = r.size
        if out is None:
            out = (np.empty((n, self.K)), np.empty(n), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.uint8))
        q, ll, it, cv = out
        self._chk(self.lib.mchip_fit_q_rows(self.h, slot, r.ctypes.data, n, int(bool(from_slot)), max_iter, abs_error, rel_error,
                                            q.ctypes.data, ll.ctypes.data, it.ctypes.data, cv.ctypes.data))
        return q, ll, it, cv

    def impute_missing(self, slot, n_real, conf=True, out=None):
        """mchip_impute_missing: the missing copies of the installed data set filled from the parameters of `slot`
        (include/multiclust_hip.h): (geno [I][L][ploidy], conf [I][L] or None, copies filled, copies left missing, genotypes
        filled, sum of the confidences).  out: (geno, conf) arrays to fill instead of new ones."""
        nr = np.ascontiguousarray(n_real, dtype=np.int32)
        assert nr.shape == (self.L,)
        if out is None:
            out = (np.empty((self.I, self.L, self.ploidy), dtype=np.uint8), np.empty((self.I, self.L)) if conf else None)
        g, c = out
        nf, nl, ng, sc = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
        self._chk(self.lib.mchip_impute_missing(self.h, slot, nr.ctypes.data, g.ctypes.data, None if c is None else c.ctypes.data,
                                                C.byref(nf), C.byref(nl), C.byref(ng), C.byref(sc)))
        return g, c, nf.value, nl.value, ng.value, sc.value

    def divergence(self, slot, weights, loci=True):
        """mchip_divergence: the divergence of the clusters of `slot` (include/multiclust_hip.h): dict with het [K], sqdiff [K][K],
        locus_v and locus_ht [L] (None without `loci`), sum_v, sum_ht, n_loci."""
        w = np.ascontiguousarray(weights, dtype=np.float64)
        assert w.shape == (self.K,)
        het, sq = np.empty(self.K), np.empty((self.K, self.K))
        lv, lht = (np.empty(self.L), np.empty(self.L)) if loci else (None, None)
        sv, sht, n1 = C.c_double(), C.c_double(), C.c_int()
        self._chk(self.lib.mchip_divergence(self.h, slot, w.ctypes.data, het.ctypes.data, sq.ctypes.data,
                                            None if lv is None else lv.ctypes.data, None if lht is None else lht.ctypes.data,
                                            C.byref(sv), C.byref(sht), C.byref(n1)))
        return dict(het=het, sqdiff=sq, locus_v=lv, locus_ht=lht, sum_v=sv.value, sum_ht=sht.value, n_loci=n1.value)

    def residual_products(self, slot, want_norms=True):
        """mchip_residual_products: the products of the admixture fit's residuals between individuals for the parameters of `slot`
        (include/multiclust_hip.h): (gram [I][I], norms [I][I] or None without `want_norms`)."""
        G = np.empty((self.I, self.I))
        D = np.empty((self.I, self.I)) if want_norms else None
        self._chk(self.lib.mchip_residual_products(self.h, slot, G.ctypes.data, None if D is None else D.ctypes.data))
        return G, D

    def kinship_products(self, slot):
        """mchip_kinship_products: the sums behind the kinship coefficients under the admixture fit in `slot`
        (include/multiclust_hip.h): (gram [I][I], scale [I][I]); phi = gram / scale, NaN where scale is 0."""
        G, V = np.empty((self.I, self.I)), np.empty((self.I, self.I))
        self._chk(self.lib.mchip_kinship_products(self.h, slot, G.ctypes.data, V.ctypes.data))
        return G, V

    def resample_loci(self, src):
        """install the selection `src` (locus indices into the base, repeats allowed) of the base: the data set held when the first
        selection was asked for; None: the base again (include/multiclust_hip.h).  Drops the model; L and T follow."""
        base = getattr(self, "_rs_ua", None)
        if base is None:
            base = getattr(self, "_ua", None)
        if src is None:
            self._chk(self.lib.mchip_resample_loci(self.h, None, 0))
            ua = base
        else:
            s = np.ascontiguousarray(src, dtype=np.int32)
            assert s.ndim == 1
            if base is None and self.L:
                raise HipError("resample_loci: this wrapper was not told the allele lists of the data set its context holds")
            self._chk(self.lib.mchip_resample_loci(self.h, s.ctypes.data, s.size))
            ua = base[s]
        self._rs_ua, self._ua = base, ua
        self.L, self.T, self.K = int(ua.size), int(ua.sum()), 0

    def set_init_genotypes(self, geno):
        """The data set hard-partition initialisations read instead of the current one (None: back to the current one)."""
        if geno is None:
            self._chk(self.lib.mchip_set_init_genotypes(self.h, None))
            return
        g = np.ascontiguousarray(geno, dtype=np.uint8)
        assert g.shape == (self.I, self.L, self.ploidy)
        self._chk(self.lib.mchip_set_init_genotypes(self.h, g.ctypes.data))

    def simulate_genotypes(self, I, L, ploidy, ua, window, K, q, p, eta_constrained=0):
        """Parametric-bootstrap data set drawn on the device (include/multiclust_hip.h); drops the model."""
        ua = np.ascontiguousarray(ua, dtype=np.int32)
        w = np.ascontiguousarray(window, dtype=np.uint32)
        q = np.ascontiguousarray(q, dtype=np.float64)
        p = np.ascontiguousarray(p, dtype=np.float64)
        assert w.size == 31 and ua.size == L and p.size == K * int(ua.sum())
        assert q.size == (K if eta_constrained else I * K)
        self._chk(self.lib.mchip_simulate_genotypes(self.h, I, L, ploidy, ua.ctypes.data, w.ctypes.data, K,
                                                    eta_constrained, q.ctypes.data, p.ctypes.data))
        self.I, self.L, self.ploidy, self.T = I, L, ploidy, int(ua.sum())
        self._ua, self._rs_ua = ua.copy(), None

    def simulate_genotypes_mixture(self, I, L, ploidy, ua, window, K, eta, p):
        """The mixture model's parametric-bootstrap data set drawn on the device (include/multiclust_hip.h); drops the model."""
        ua = np.ascontiguousarray(ua, dtype=np.int32)
        w = np.ascontiguousarray(window, dtype=np.uint32)
        eta = np.ascontiguousarray(eta, dtype=np.float64)
        p = np.ascontiguousarray(p, dtype=np.float64)
        assert w.size == 31 and ua.size == L and p.size == K * int(ua.sum()) and eta.size == K
        self._chk(self.lib.mchip_simulate_genotypes_mixture(self.h, I, L, ploidy, ua.ctypes.data, w.ctypes.data, K,
                                                            eta.ctypes.data, p.ctypes.data))
        self.I, self.L, self.ploidy, self.T = I, L, ploidy, int(ua.sum())
        self._ua, self._rs_ua = ua.copy(), None

    def init_from_individual_centers(self, centers, to=0):
        """Mixture model: assignment to the nearest of the K center individuals and the parameters initialised from it, into
        slot `to`; returns the assignment [I]."""
        c = np.ascontiguousarray(centers, dtype=np.int32)
        assert c.size == self.K
        out = np.empty(self.I, dtype=np.int32)
        self._chk(self.lib.mchip_init_from_individual_centers(self.h, c.ctypes.data, to, out.ctypes.data))
        return out

    def set_model(self, K, admixture=1, eta_constrained=0, do_projection=1, lower_bound=1e-8, n_secants=1):
        self._chk(self.lib.mchip_set_model(self.h, K, admixture, eta_constrained, do_projection,
                                           lower_bound, lower_bound, n_secants))
        self.K = K
        self.indiv_q = bool(admixture and not eta_constrained)

    def set_p(self, slot, p):
        p = np.ascontiguousarray(p, dtype=np.float64)
        assert p.size == self.K * self.T
        self._chk(self.lib.mchip_set_p(self.h, slot, p.ctypes.data))

    def get_p(self, slot):
        p = np.empty((self.K, self.T), dtype=np.float64)
        self._chk(self.lib.mchip_get_p(self.h, slot, p.ctypes.data))
        return p

    def set_q(self, slot, q):
        q = np.ascontiguousarray(q, dtype=np.float64)
        assert q.size == (self.I * self.K if self.indiv_q else self.K)
        self._chk(self.lib.mchip_set_q(self.h, slot, q.ctypes.data))

    def get_q(self, slot):
        q = np.empty((self.I, self.K) if self.indiv_q else (self.K,), dtype=np.float64)
        self._chk(self.lib.mchip_get_q(self.h, slot, q.ctypes.data))
        return q

    def em_step(self, frm=0, to=0, sync=True):
        if not sync:
            self._chk(self.lib.mchip_em_step(self.h, frm, to, None))
            return None
        ll = C.c_double()
        self._chk(self.lib.mchip_em_step(self.h, frm, to, C.byref(ll)))
        return ll.value

    def last_loglik(self):
        ll = C.c_double()
        self._chk(self.lib.mchip_last_loglik(self.h, C.byref(ll)))
        return ll.value

    def e_step(self, slot=0):
        ll = C.c_double()
        self._chk(self.lib.mchip_e_step(self.h, slot, C.byref(ll)))
        return ll.value

    def loglik(self, slot=0, sync=True):
        if not sync:
            self._chk(self.lib.mchip_loglik(self.h, slot, None))
            return None
        ll = C.c_double()
        self._chk(self.lib.mchip_loglik(self.h, slot, C.byref(ll)))
        return ll.value

    def loglik_prefetch(self, slot=0):
        ll = C.c_double()
        self._chk(self.lib.mchip_loglik_prefetch(self.h, slot, C.byref(ll)))
        return ll.value

    def mstep_from_partition(self, assign, to=0):
        a = np.ascontiguousarray(assign, dtype=np.uint8)
        assert a.size == self.I * self.L * self.ploidy
        self._chk(self.lib.mchip_mstep_from_partition(self.h, a.ctypes.data, to))

    def mstep_from_rand_partition(self, window, to=0):
        """window: the 31 uint32 words behind the first draw, oldest first (see include/multiclust_hip.h)."""
        w = np.ascontiguousarray(window, dtype=np.uint32)
        assert w.size == 31
        self._chk(self.lib.mchip_mstep_from_rand_partition(self.h, w.ctypes.data, to))

    def expected_counts(self):
        s = np.empty((self.I, self.K), dtype=np.float64)
        self._chk(self.lib.mchip_get_expected_counts(self.h, s.ctypes.data))
        return s

    def secant(self, which, j, to, frm):
        self._chk(self.lib.mchip_secant(self.h, which, j, to, frm))

    def step_dots(self, j):
        out = (C.c_double * 3)()
        self._chk(self.lib.mchip_step_dots(self.h, j, out))
        return list(out)

    def secant_dots(self, j1, j2):
        out = (C.c_double * 2)()
        self._chk(self.lib.mchip_secant_dots(self.h, j1, j2, out))
        return list(out)

    def accel_update(self, to, base, j, s, qn_form=0):
        self._chk(self.lib.mchip_accel_update(self.h, to, base, j, s, qn_form))

    def set_secant(self, which, j, p_part, q_part):
        """secant buffer j (which = 0: u, 1: v) written whole, in the boundary's flat order: P part [K][T], Q part [I][K] or [K]"""
        p = np.ascontiguousarray(p_part, dtype=np.float64)
        q = np.ascontiguousarray(q_part, dtype=np.float64)
        assert p.size == self.K * self.T and q.size == (self.I * self.K if self.indiv_q else self.K)
        self._chk(self.lib.mchip_set_secant(self.h, which, j, p.ctypes.data, q.ctypes.data))

    def get_secant(self, which, j):
        """(P part [K][T], Q part [I][K] or [K]) of secant buffer j (which = 0: u, 1: v)"""
        p = np.empty((self.K, self.T), dtype=np.float64)
        q = np.empty((self.I, self.K) if self.indiv_q else (self.K,), dtype=np.float64)
        self._chk(self.lib.mchip_get_secant(self.h, which, j, p.ctypes.data, q.ctypes.data))
        return p, q

    def multisecant_update(self, to, base, u_index, v_index=(), coef_a=(), coef_b=()):
        """x[to] = x[base] + u[u_index], then += v[v_index[t]] * coef_a[t] * coef_b[t] term by term, projected"""
        vi = np.ascontiguousarray(v_index, dtype=np.int32)
        ca = np.ascontiguousarray(coef_a, dtype=np.float64)
        cb = np.ascontiguousarray(coef_b, dtype=np.float64)
        assert vi.ndim == 1 and vi.size == ca.size == cb.size
        n = int(vi.size)
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        self._chk(self.lib.mchip_multisecant_update(self.h, to, base, u_index, n, vi.ctypes.data_as(ip) if n else None,
                                                    ca.ctypes.data_as(dp) if n else None, cb.ctypes.data_as(dp) if n else None))

    def synchronize(self):
        self._chk(self.lib.mchip_synchronize(self.h))

    def profile_begin(self):
        self._chk(self.lib.mchip_profile_begin(self.h))

    def profile_end(self):
        total = C.c_double()
        km = (C.c_double * PROF_KINDS)()
        kl = (C.c_int * PROF_KINDS)()
        self._chk(self.lib.mchip_profile_end(self.h, C.byref(total), km, kl))
        return total.value, list(km), list(kl)

    def device_info(self):
        name = C.create_string_buffer(256)
        cu = C.c_int()
        mem = C.c_double()
        self._chk(self.lib.mchip_device_info(self.h, name, 256, C.byref(cu), C.byref(mem)))
        return name.value.decode(), cu.value, mem.value
