"""ctypes view of multiclust_amd/host/mc_host.h (libmulticlust_host.so): the plain-C host side that mirrors
the reference's em()/em_step()/stop()/accelerated_em_step() over the C-ABI."""
import ctypes as C
import os

import numpy as np

from . import hip

_HERE = os.path.dirname(os.path.abspath(__file__))


class McOptions(C.Structure):
    _fields_ = [("admixture", C.c_int), ("eta_constrained", C.c_int), ("do_projection", C.c_int),
                ("accel_scheme", C.c_int), ("q", C.c_int), ("n_init_iter", C.c_int), ("max_iter", C.c_int),
                ("n_seconds", C.c_uint), ("adjust_step", C.c_int), ("verbosity", C.c_int),
                ("abs_error", C.c_double), ("rel_error", C.c_double), ("lower_bound", C.c_double),
                ("eta_lower_bound", C.c_double), ("p_lower_bound", C.c_double), ("seed", C.c_uint),
                ("initialization_procedure", C.c_int), ("n_rand_em_init", C.c_int)]


class McData(C.Structure):
    _fields_ = [("I", C.c_int), ("L", C.c_int), ("ploidy", C.c_int),
                ("uniquealleles", C.c_void_p), ("geno", C.c_void_p), ("init_geno", C.c_void_p),
                ("bed", C.c_void_p), ("bed_record_bytes", C.c_size_t), ("lazy", C.c_void_p)]


class McModel(C.Structure):
    _fields_ = [("K", C.c_int), ("pindex", C.c_int), ("findex", C.c_int), ("tindex", C.c_int),
                ("delta_index", C.c_int), ("logL", C.c_double), ("n_iter", C.c_int), ("converged", C.c_int),
                ("stopped", C.c_int), ("accel_step", C.c_int), ("iter_stop", C.c_int), ("time_stop", C.c_int),
                ("fatal", C.c_int), ("start", C.c_long), ("seconds_run", C.c_double),
                ("A", C.c_double * 9), ("Ainv", C.c_double * 9), ("cutu", C.c_double * 3),
                ("last_emll", C.c_double), ("last_step", C.c_double), ("last_ll", C.c_double),
                ("last_accepted", C.c_int), ("dev", C.c_void_p), ("owns_dev", C.c_int), ("init_cache", C.c_void_p)]


class McRng(C.Structure):
    _fields_ = [("r", C.c_int32 * 31), ("f", C.c_int), ("b", C.c_int)]


class McSimulation(C.Structure):
    _fields_ = [("window", C.c_uint32 * 31), ("K", C.c_int), ("q", C.c_void_p), ("p", C.c_void_p)]


class McUnitResult(C.Structure):
    _fields_ = [("unit", C.c_int), ("logL", C.c_double), ("converged", C.c_int), ("n_iter", C.c_int),
                ("time_stop", C.c_int), ("iter_stop", C.c_int), ("pindex", C.c_int), ("fatal", C.c_int),
                ("seconds_run", C.c_double)]


class McReplicateResult(C.Structure):
    _fields_ = [("replicate", C.c_int), ("logL_H0", C.c_double), ("logL_HA", C.c_double), ("ts", C.c_double),
                ("n_iter", C.c_int), ("fatal", C.c_int)]


class McSummary(C.Structure):
    _fields_ = [("n_init", C.c_int), ("n_total_iter", C.c_int), ("n_max_iter", C.c_int),
                ("n_maxll_times", C.c_int), ("n_maxll_init", C.c_int), ("ever_converged", C.c_int),
                ("best_unit", C.c_int), ("max_logL", C.c_double), ("first_max_logL", C.c_double),
                ("aic", C.c_double), ("bic", C.c_double)]


CV_MAX_FOLDS = 64


class McCvResult(C.Structure):
    """mc_cv_result (multiclust_amd/host/mc_host.h)"""
    _fields_ = [("cv", C.c_double), ("sum_log", C.c_double), ("floor", C.c_double), ("n_copies", C.c_uint64),
                ("n_floored", C.c_uint64), ("n_folds", C.c_int), ("fatal_fold", C.c_int),
                ("fold_sum_log", C.c_double * CV_MAX_FOLDS), ("fold_copies", C.c_uint64 * CV_MAX_FOLDS),
                ("fold_floored", C.c_uint64 * CV_MAX_FOLDS), ("fold_iter", C.c_int * CV_MAX_FOLDS)]


class McSeResult(C.Structure):
    """mc_se_result (multiclust_amd/host/mc_host.h)"""
    _fields_ = [("n_replicates", C.c_int), ("block", C.c_int), ("n_failed", C.c_int), ("n_iter", C.c_uint64),
                ("mean_se", C.c_double), ("max_se", C.c_double)]


class McQueryResult(C.Structure):
    """mc_query_result (multiclust_amd/host/mc_host.h)"""
    _fields_ = [("n", C.c_int), ("K", C.c_int), ("n_converged", C.c_int), ("n_failed", C.c_int), ("max_iter", C.c_int),
                ("sum_logL", C.c_double), ("rows", C.POINTER(C.c_int32)), ("iter", C.POINTER(C.c_int32)),
                ("q", C.POINTER(C.c_double)), ("logL", C.POINTER(C.c_double)), ("converged", C.POINTER(C.c_uint8))]


class McImputeResult(C.Structure):
    """mc_impute_result (multiclust_amd/host/mc_host.h)"""
    _fields_ = [("n_filled", C.c_uint64), ("n_left", C.c_uint64), ("n_genotypes", C.c_uint64), ("sum_conf", C.c_double),
                ("mean_conf", C.c_double)]


class McDivergenceResult(C.Structure):
    """mc_divergence_result (multiclust_amd/host/mc_host.h)"""
    _fields_ = [("K", C.c_int), ("L", C.c_int), ("n_loci", C.c_int), ("n_pairs", C.c_int), ("f_mean", C.c_double),
                ("f_min", C.c_double), ("f_max", C.c_double), ("sum_v", C.c_double), ("sum_ht", C.c_double), ("f_all", C.c_double),
                ("w", C.POINTER(C.c_double)), ("H", C.POINTER(C.c_double)), ("D", C.POINTER(C.c_double)),
                ("F", C.POINTER(C.c_double)), ("locus_ht", C.POINTER(C.c_double)), ("locus_f", C.POINTER(C.c_double))]


class McResidResult(C.Structure):
    """mc_resid_result (multiclust_amd/host/mc_host.h)"""
    _fields_ = [("K", C.c_int), ("I", C.c_int), ("max_i", C.c_int), ("max_j", C.c_int), ("n_pairs", C.c_longlong),
                ("mean", C.c_double), ("mean_abs", C.c_double), ("max", C.c_double), ("cor", C.POINTER(C.c_double)),
                ("ind_mean", C.POINTER(C.c_double)), ("ind_max", C.POINTER(C.c_double)), ("ind_partner", C.POINTER(C.c_int32))]


class CliOptions(C.Structure):
    """mc_cli_options (multiclust_amd/host/mc_cli.h)"""
    _fields_ = [("em", McOptions), ("filename", C.c_char_p), ("filename_file", C.c_char_p), ("path", C.c_char_p),
                ("outfile_name", C.c_char_p), ("min_K", C.c_int), ("max_K", C.c_int), ("n_init", C.c_int),
                ("n_bootstrap", C.c_int), ("n_rand_em_init", C.c_int), ("missing_value", C.c_int), ("R_format", C.c_int),
                ("ploidy", C.c_int), ("seed_given", C.c_int), ("target_ll", C.c_int), ("target_revisit", C.c_int),
                ("desired_ll", C.c_double), ("n_repeat", C.c_int), ("repeat_seconds", C.c_uint),
                ("max_repeat_seconds", C.c_uint), ("write_files", C.c_int), ("compact", C.c_int), ("parallel", C.c_int),
                ("device", C.c_int), ("n_gpus", C.c_int), ("n_streams", C.c_int), ("pfile", C.c_char_p), ("qfile", C.c_char_p),
                ("afile", C.c_char_p), ("bed_prefix", C.c_char_p)]
    # (the C struct goes on: CliOptionsAll)


class CliOptionsAll(CliOptions):
    """the whole of mc_cli_options: what the readers and writers are handed, since mc_read_bed reads the last fields"""
    _fields_ = [  # the command line's --cv, --se, --query, --fill, --fst and --resid: only the binary (mc_main.c, mc_cli_*.c) reads them
                ("cv_folds", C.c_int), ("cv_floor", C.c_double), ("se_replicates", C.c_int), ("se_block", C.c_int),
                ("query_file", C.c_char_p), ("fill", C.c_int), ("fst", C.c_int), ("resid", C.c_int),
                # --prune / --prune-window
                ("prune", C.c_int), ("prune_window_given", C.c_int), ("prune_t", C.c_double), ("prune_window", C.c_int),
                # --king-cutoff
                ("king", C.c_int), ("king_t", C.c_double),
                # --mind, --geno, --maf, --hwe
                ("mind", C.c_int), ("geno", C.c_int), ("maf", C.c_int), ("hwe", C.c_int), ("mind_t", C.c_double),
                ("geno_t", C.c_double), ("maf_t", C.c_double), ("hwe_t", C.c_double),
                # --pca, --pca-iter, --pca-tol
                ("pca", C.c_int), ("pca_iter", C.c_int), ("pca_tol", C.c_double),
                # --kinship
                ("kinship", C.c_int), ("kinship_t", C.c_double)]


class McKingPair(C.Structure):
    """mc_king_pair (multiclust_amd/host/mc_cli.h)"""
    _fields_ = [("i", C.c_int), ("j", C.c_int), ("n", C.c_uint32), ("hh", C.c_uint32), ("op", C.c_uint32), ("phi", C.c_double)]


class CliData(C.Structure):
    """mc_cli_data (multiclust_amd/host/mc_cli.h)"""
    _fields_ = [("I", C.c_int), ("L", C.c_int), ("ploidy", C.c_int), ("M", C.c_int), ("missing_data", C.c_int),
                ("interleaved", C.c_int), ("IL", C.POINTER(C.c_int)), ("uniquealleles", C.POINTER(C.c_int32)),
                ("L_alleles", C.POINTER(C.POINTER(C.c_int))), ("geno", C.POINTER(C.c_uint8)),
                ("names", C.POINTER(C.c_char_p)), ("locale", C.POINTER(C.c_int)), ("pops", C.POINTER(C.c_char_p)),
                ("numpops", C.c_int), ("i_p", C.POINTER(C.c_int)), ("T", C.c_int), ("toff", C.POINTER(C.c_int32)),
                ("bed", C.POINTER(C.c_uint8)), ("bed_record_bytes", C.c_size_t), ("lazy", C.c_void_p)]
    # (the C struct goes on: CliDataAll)


class CliDataAll(CliData):
    """the whole of mc_cli_data: what the readers fill (they clear all of it) and the writers read"""
    _fields_ = [("L_file", C.c_int), ("bim_text", C.c_void_p), ("chrom", C.POINTER(C.c_char_p)),
                ("variant_id", C.POINTER(C.c_char_p)), ("variant_of", C.POINTER(C.c_int)),
                ("I_file", C.c_int), ("individual_of", C.POINTER(C.c_int)), ("fam_fid", C.POINTER(C.c_char_p)),
                ("fam_iid", C.POINTER(C.c_char_p)), ("king_pairs", C.POINTER(McKingPair)), ("n_king_pairs", C.c_size_t),
                ("filters_run", C.c_int), ("qc", C.c_void_p)]


def _cli_data_fields(d, geno):
    """what both readers fill alike; L_alleles (the real alleles of every locus: uniquealleles less the phantom slot of a locus
    with a missing copy) needs the genotype to know its lengths and is left out without it"""
    ua = np.ctypeslib.as_array(d.uniquealleles, shape=(d.L,)).copy()
    extra = {}
    if geno is not None:
        n_real = ua - ((geno == 0xFF).any(axis=(0, 2)) & (ua > 0))
        extra["L_alleles"] = [[d.L_alleles[l][m] for m in range(int(n_real[l]))] for l in range(d.L)]
    return dict(extra, I=d.I, L=d.L, ploidy=d.ploidy, T=d.T, M=d.M, missing_data=d.missing_data, interleaved=d.interleaved, ua=ua,
                toff=np.ctypeslib.as_array(d.toff, shape=(d.L + 1,)).copy(),
                locale=np.ctypeslib.as_array(d.locale, shape=(d.I,)).copy(), numpops=d.numpops,
                names=[d.names[i].decode() for i in range(d.I)], pops=[d.pops[i].decode() for i in range(d.numpops)],
                i_p=[d.i_p[n] for n in range(d.numpops)])


def read_structure(path, ploidy=2, missing=-9, r_format=0):
    """mc_read_structure (host/mc_reader.c; reference read_file.c:38-300, 443-663) on a STRUCTURE file: (status, None) on
    failure, else (0, dict of the fields the EM path and the writers read)."""
    lib = load()
    lib.mc_read_structure.argtypes = [C.POINTER(CliOptionsAll), C.POINTER(CliDataAll)]
    lib.mc_free_data.argtypes = [C.POINTER(CliDataAll)]
    o = CliOptionsAll()
    o.filename = path.encode()
    o.ploidy, o.missing_value, o.R_format = ploidy, missing, r_format
    d = CliDataAll()
    rc = lib.mc_read_structure(C.byref(o), C.byref(d))
    if rc:
        return rc, None
    geno = np.ctypeslib.as_array(d.geno, shape=(d.I, d.L, d.ploidy)).copy()
    out = _cli_data_fields(d, geno)
    out["geno"] = geno
    lib.mc_free_data(C.byref(d))
    return 0, out


def bed_decode(I, bed):
    """mc_bed_decode (host/mc_bed.c), the CPU form of the device's unpacking: packed records [L][record_bytes] ->
    (uniquealleles [L], geno [I][L][2]) of the equivalent STRUCTURE file."""
    lib = load()
    lib.mc_bed_decode.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.mc_bed_decode.restype = None
    bed = np.ascontiguousarray(bed, dtype=np.uint8)
    assert bed.ndim == 2 and bed.shape[1] >= (I + 3) // 4
    L = bed.shape[0]
    ua = np.empty(L, dtype=np.int32)
    geno = np.empty((I, L, 2), dtype=np.uint8)
    lib.mc_bed_decode(I, L, bed.ctypes.data, bed.shape[1], ua.ctypes.data, geno.ctypes.data)
    return ua, geno


def read_bed(prefix, decode=True, prune=None, prune_window=50, device=0, king_cutoff=None):
    """mc_read_bed (host/mc_bed.c) on the PLINK 1 fileset prefix.bed/.bim/.fam: (status, None) on failure, else (0, dict) with
    the fields of read_structure.  The reader keeps the data set packed -- `bed` [L][record_bytes], geno_is_null says that it
    built no genotype; `geno` (and L_alleles) come from mc_bed_decode on those records, unless decode is False.  chrom and
    variant_id are the first two fields of the L_file lines of the .bim.  prune = t: the variants thinned by linkage disequilibrium
    on `device` as --prune t --prune-window prune_window does (host/mc_ld.c): everything is the pruned data set's, variant_of its
    loci's places in the fileset (None without pruning).  king_cutoff = t: after that, close relatives removed on `device` as
    --king-cutoff t does (host/mc_king.c): everything is the kept individuals', individual_of their places in the fileset (None
    without it), I_file, fam_fid, fam_iid the fileset's, king_pairs the related pairs as (i, j, n, hh, op, phi)."""
    lib = load()
    lib.mc_read_bed.argtypes = [C.POINTER(CliOptionsAll), C.POINTER(CliDataAll)]
    lib.mc_free_data.argtypes = [C.POINTER(CliDataAll)]
    o = CliOptionsAll()
    o.bed_prefix = prefix.encode()
    o.ploidy = 2
    d = CliDataAll()
    rc = lib.mc_read_bed(C.byref(o), C.byref(d))
    if rc:
        return rc, None
    if prune is not None:
        lib.mc_ld_prune_data.argtypes = [C.POINTER(CliOptionsAll), C.POINTER(CliDataAll)]
        o.device, o.prune, o.prune_t, o.prune_window = device, 1, prune, prune_window
        rc = lib.mc_ld_prune_data(C.byref(o), C.byref(d))
        if rc:
            lib.mc_free_data(C.byref(d))
            return rc, None
    if king_cutoff is not None:
        lib.mc_king_data.argtypes = [C.POINTER(CliOptionsAll), C.POINTER(CliDataAll)]
        o.device, o.king, o.king_t = device, 1, king_cutoff
        rc = lib.mc_king_data(C.byref(o), C.byref(d))
        if rc:
            lib.mc_free_data(C.byref(d))
            return rc, None
    bed = np.ctypeslib.as_array(d.bed, shape=(d.L, d.bed_record_bytes)).copy()
    geno = ua_dec = None
    if decode:
        ua_dec, geno = bed_decode(d.I, bed)
    out = _cli_data_fields(d, geno)
    out.update(geno_is_null=not bool(d.geno), bed=bed, L_file=d.L_file, chrom=[d.chrom[v].decode() for v in range(d.L_file)],
               variant_id=[d.variant_id[v].decode() for v in range(d.L_file)],
               variant_of=[d.variant_of[l] for l in range(d.L)] if d.variant_of else None,
               individual_of=[d.individual_of[i] for i in range(d.I)] if d.individual_of else None)
    if d.individual_of:
        out.update(I_file=d.I_file, fam_fid=[d.fam_fid[i].decode() for i in range(d.I_file)],
                   fam_iid=[d.fam_iid[i].decode() for i in range(d.I_file)],
                   king_pairs=[(k.i, k.j, k.n, k.hh, k.op, k.phi) for k in (d.king_pairs[x] for x in range(d.n_king_pairs))])
    if decode:
        out.update(geno=geno, ua_decoded=ua_dec)
    lib.mc_free_data(C.byref(d))
    return 0, out


def write_filled_structure(path, out_path, filled, ploidy=2, missing=-9, r_format=0):
    """mc_write_filled_structure (host/mc_impute.c): the STRUCTURE file `path`, read with these reader options, copied to out_path
    with every missing allele token whose copy is not 0xFF in filled [I][L][ploidy] replaced by that allele's label; returns the
    status (0 = written)."""
    lib = load()
    o = CliOptionsAll()
    o.filename = path.encode()
    o.ploidy, o.missing_value, o.R_format = ploidy, missing, r_format
    d = CliDataAll()
    rc = lib.mc_read_structure(C.byref(o), C.byref(d))
    if rc:
        return rc
    f = np.ascontiguousarray(filled, dtype=np.uint8)
    assert f.shape == (d.I, d.L, d.ploidy)
    rc = lib.mc_write_filled_structure(C.byref(o), C.byref(d), f.ctypes.data, out_path.encode())
    lib.mc_free_data(C.byref(d))
    return rc


def write_filled_bed(prefix, out_prefix, filled):
    """mc_write_filled_bed (host/mc_impute.c): the PLINK fileset `prefix` copied to out_prefix.bed/.bim/.fam with every missing
    record whose two copies are not 0xFF in filled [I][L][2] replaced by the genotype they spell; returns the status."""
    lib = load()
    o = CliOptionsAll()
    o.bed_prefix = prefix.encode()
    o.ploidy = 2
    d = CliDataAll()
    rc = lib.mc_read_bed(C.byref(o), C.byref(d))
    if rc:
        return rc
    f = np.ascontiguousarray(filled, dtype=np.uint8)
    assert f.shape == (d.I, d.L, 2)
    rc = lib.mc_write_filled_bed(C.byref(o), C.byref(d), f.ctypes.data, out_prefix.encode())
    lib.mc_free_data(C.byref(d))
    return rc


def impute_n_real(ua, geno=None, bed=None, I=None):
    """mc_impute_n_real (host/mc_impute.c): the candidate alleles of every locus, uniquealleles[l] without the phantom slot, from
    the genotype [I][L][ploidy] or from packed PLINK records [L][record_bytes] of I individuals"""
    lib = load()
    ua = np.ascontiguousarray(ua, dtype=np.int32)
    if geno is not None:
        g = np.ascontiguousarray(geno, dtype=np.uint8)
        dat = McData(g.shape[0], g.shape[1], g.shape[2], ua.ctypes.data, g.ctypes.data)
    else:
        b = np.ascontiguousarray(bed, dtype=np.uint8)
        dat = McData(I, b.shape[0], 2, ua.ctypes.data, None, None, b.ctypes.data, b.shape[1])
    out = np.empty(ua.size, dtype=np.int32)
    if lib.mc_impute_n_real(C.byref(dat), out.ctypes.data):
        raise hip.HipError("mc_impute_n_real failed")
    return out


def divergence_weights(q, K):
    """mc_divergence_weights (host/mc_diverge.c): the weights --fst gives the clusters from a fit's Q: the column means of q [I][K]
    over the rows without a NaN (1 / K when there is none), or q [K] itself"""
    q = np.ascontiguousarray(q, dtype=np.float64)
    w = np.empty(K)
    load().mc_divergence_weights(K, q.shape[0] if q.ndim == 2 else 0, q.ctypes.data, w.ctypes.data)
    return w


def divergence_tables(het, sqdiff, n_loci):
    """mc_divergence_tables and mc_divergence_summary (host/mc_diverge.c): (H [K], D [K][K], F [K][K], (pairs with a number,
    their mean, smallest, largest F)) from the device's sums"""
    het = np.ascontiguousarray(het, dtype=np.float64)
    sq = np.ascontiguousarray(sqdiff, dtype=np.float64)
    K = het.size
    H, D, F = np.empty(K), np.empty((K, K)), np.empty((K, K))
    lib = load()
    lib.mc_divergence_tables(K, n_loci, het.ctypes.data, sq.ctypes.data, H.ctypes.data, D.ctypes.data, F.ctypes.data)
    n, mean, lo, hi = C.c_int(), C.c_double(), C.c_double(), C.c_double()
    lib.mc_divergence_summary(K, F.ctypes.data, C.byref(n), C.byref(mean), C.byref(lo), C.byref(hi))
    return H, D, F, (n.value, mean.value, lo.value, hi.value)


def residual_ratios(G, D):
    """mc_residual_ratios (host/mc_resid.c): cor [I][I] = G_ij / sqrt(D_ij D_ji), NaN on the diagonal and where either D is 0"""
    G = np.ascontiguousarray(G, dtype=np.float64)
    D = np.ascontiguousarray(D, dtype=np.float64)
    I = G.shape[0]
    assert G.shape == D.shape == (I, I)
    cor = np.empty((I, I))
    load().mc_residual_ratios(I, G.ctypes.data, D.ctypes.data, cor.ctypes.data)
    return cor


def _resid_dict(r):
    I = r.I
    return dict(cor=np.ctypeslib.as_array(r.cor, shape=(I, I)).copy(), ind_mean=np.ctypeslib.as_array(r.ind_mean, shape=(I,)).copy(),
                ind_max=np.ctypeslib.as_array(r.ind_max, shape=(I,)).copy(),
                ind_partner=np.ctypeslib.as_array(r.ind_partner, shape=(I,)).copy(), n_pairs=r.n_pairs, mean=r.mean,
                mean_abs=r.mean_abs, max=r.max, max_pair=(r.max_i, r.max_j))


def residual_summary(cor):
    """mc_residual_summary (host/mc_resid.c) of a correlation matrix: dict as Fit.residual_correlation gives it"""
    cor = np.ascontiguousarray(cor, dtype=np.float64)
    I = cor.shape[0]
    im, ix, ip = np.empty(I), np.empty(I), np.empty(I, dtype=np.int32)
    r = McResidResult(I=I, cor=cor.ctypes.data_as(C.POINTER(C.c_double)), ind_mean=im.ctypes.data_as(C.POINTER(C.c_double)),
                      ind_max=ix.ctypes.data_as(C.POINTER(C.c_double)), ind_partner=ip.ctypes.data_as(C.POINTER(C.c_int32)))
    load().mc_residual_summary(I, cor.ctypes.data, C.byref(r))
    return _resid_dict(r)


def king_select(bits, I):
    """mc_king_select (host/mc_king.c): keep [I] bool under the greedy rule on the relatedness graph bits [I][I] (bool, symmetric)"""
    lib = load()
    rel = np.asarray(bits, dtype=bool)
    assert rel.shape == (I, I)
    rw = (I + 63) // 64
    packed = np.zeros((I, rw * 64), dtype=np.uint8)
    packed[:, :I] = rel
    words = np.packbits(packed, axis=1, bitorder="little").view(np.uint64).reshape(I, rw).copy()
    keep = np.empty(I, dtype=np.uint8)
    lib.mc_king_select.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    rc = lib.mc_king_select(I, words.ctypes.data, keep.ctypes.data)
    if rc:
        raise hip.HipError("mc_king_select failed (%d)" % rc)
    return keep.astype(bool)


def king_compact(I, bed, keep):
    """mc_king_compact (host/mc_king.c): (records [L][ceil(I'/4)] of the kept individuals, individual_of [I'])"""
    lib = load()
    bed = np.ascontiguousarray(bed, dtype=np.uint8)
    L, rb = bed.shape
    buf = np.zeros(L * rb + 8, dtype=np.uint8)
    buf[:L * rb] = bed.ravel()
    k = np.ascontiguousarray(keep, dtype=np.uint8)
    assert k.shape == (I,)
    of = np.empty(I, dtype=np.int32)
    lib.mc_king_compact.argtypes = [C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    n = lib.mc_king_compact(I, L, rb, k.ctypes.data, buf.ctypes.data, of.ctypes.data)
    if n < 0:
        raise hip.HipError("mc_king_compact failed")
    return buf[:L * ((n + 3) // 4)].reshape(L, (n + 3) // 4).copy(), of[:n].copy()


def query_read(path, I):
    """mc_query_read (host/mc_query.c) on a query file: (status, None) on failure, else (0, mask [I] uint8)"""
    lib = load()
    m = C.POINTER(C.c_uint8)()
    rc = lib.mc_query_read(path.encode(), I, C.byref(m))
    if rc:
        return rc, None
    mask = np.ctypeslib.as_array(m, shape=(I,)).copy()
    _libc_free(m)
    return 0, mask


def _libc_free(ptr):
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free.restype = None
    libc.free(C.cast(ptr, C.c_void_p))


def replicate_starts(opt, dat, base, n_replicates, null_K, alt_K, n_init):
    """mc_replicate_starts: the generator at the start of every bootstrap replicate, [n_replicates + 1] McRng"""
    starts = (McRng * (n_replicates + 1))()
    rc = load().mc_replicate_starts(C.byref(opt), C.byref(dat), C.byref(base), n_replicates, null_K, alt_K, n_init, starts)
    if rc:
        raise hip.HipError("mc_replicate_starts failed (%d)" % rc)
    return starts


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    hip.load()      # dependency; raises loudly if the HIP library is missing
    path = os.path.join(_HERE, "lib", "libmulticlust_host.so")
    if not os.path.exists(path):
        raise hip.HipError("%s is missing: run `make`" % path)
    lib = C.CDLL(path)
    OP, DP, MP = C.POINTER(McOptions), C.POINTER(McData), C.POINTER(McModel)
    lib.mc_make_options.argtypes = [OP]
    lib.mc_synchronize.argtypes = [OP, DP]
    lib.mc_model_create.argtypes = [C.POINTER(MP), OP, DP, C.c_int, C.c_int]
    lib.mc_model_free.argtypes = [MP]
    for fn in ("mc_model_set_p", "mc_model_get_p", "mc_model_set_q", "mc_model_get_q"):
        getattr(lib, fn).argtypes = [MP, C.c_int, C.c_void_p]
    lib.mc_model_get_expected_counts.argtypes = [MP, C.c_void_p]
    lib.mc_initialize_model.argtypes = [OP, DP, MP, C.POINTER(McRng)]
    lib.mc_reset_model_state.argtypes = [MP]
    lib.mc_skip_initializations.argtypes = [OP, DP, MP, C.POINTER(McRng), C.c_int]
    lib.mc_em.argtypes = [OP, DP, MP]
    lib.mc_em.restype = None
    lib.mc_em_step.argtypes = [OP, DP, MP]
    lib.mc_em_e_step.argtypes = [OP, DP, MP]
    lib.mc_em_e_step.restype = C.c_double
    lib.mc_em_2_steps.argtypes = [MP, DP, OP]
    lib.mc_accelerated_em_step.argtypes = [OP, DP, MP]
    lib.mc_log_likelihood.argtypes = [OP, DP, MP, C.c_int]
    lib.mc_log_likelihood.restype = C.c_double
    lib.mc_step_size.argtypes = [OP, DP, MP]
    lib.mc_step_size.restype = C.c_double
    lib.mc_accelerated_update.argtypes = [OP, DP, MP, C.c_double]
    lib.mc_accelerated_update.restype = C.c_double
    lib.mc_srand.argtypes = [C.POINTER(McRng), C.c_uint]
    lib.mc_rand.argtypes = [C.POINTER(McRng)]
    lib.mc_rng_jump.argtypes = [C.POINTER(McRng), C.c_uint64]
    lib.mc_summary_reset.argtypes = [C.POINTER(McSummary)]
    lib.mc_summary_add.argtypes = [OP, C.POINTER(McSummary), C.POINTER(McUnitResult), C.c_int, C.c_int]
    lib.mc_draws_per_init.argtypes = [OP, DP, C.c_int]
    lib.mc_draws_per_init.restype = C.c_uint64
    lib.mc_fit_unit.argtypes = [OP, DP, MP, C.c_uint, C.c_int, C.POINTER(McUnitResult)]
    lib.mc_no_parameters.argtypes = [OP, DP, C.c_int]
    lib.mc_bootstrap_genotypes.argtypes = [OP, DP, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(McRng), C.c_void_p]
    lib.mc_bootstrap_genotypes.restype = None
    lib.mc_bootstrap_draws.argtypes = [OP, DP]
    lib.mc_bootstrap_draws.restype = C.c_uint64
    lib.mc_simulation_begin.argtypes = [C.POINTER(McSimulation), OP, DP, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(McRng)]
    lib.mc_simulation_begin.restype = None
    lib.mc_model_create_simulated.argtypes = [C.POINTER(MP), OP, DP, C.c_int, C.c_int, C.POINTER(McSimulation)]
    lib.mc_model_get_genotypes.argtypes = [MP, C.c_void_p]
    lib.mc_fit_replicate.argtypes = [OP, DP, C.c_int, C.POINTER(McRng), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p, C.POINTER(McReplicateResult), C.POINTER(MP)]
    lib.mc_replicate_starts.argtypes = [OP, DP, C.POINTER(McRng), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(McRng)]
    lib.mc_replicate_start.argtypes = [OP, DP, C.POINTER(McRng), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(McRng)]
    lib.mc_test_center_walk.argtypes = [C.c_int, C.c_int, C.POINTER(McRng), C.POINTER(C.c_int)]
    lib.mc_test_center_walk.restype = None
    lib.mc_cross_validate.argtypes = [OP, DP, MP, C.c_int, C.c_double, C.POINTER(McCvResult)]
    lib.mc_cv_default_floor.argtypes = [DP]
    lib.mc_cv_default_floor.restype = C.c_double
    lib.mc_locus_bootstrap.argtypes = [OP, DP, MP, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(McSeResult)]
    lib.mc_se_list_capacity.argtypes = [C.c_int, C.c_int]
    lib.mc_se_draw_lists.argtypes = [C.POINTER(McRng), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.mc_query_read.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.POINTER(C.c_uint8))]
    lib.mc_query_hide.argtypes = [MP, DP, C.c_void_p]
    lib.mc_query_fit.argtypes = [OP, DP, MP, C.c_void_p, C.POINTER(McQueryResult)]
    lib.mc_query_result_free.argtypes = [C.POINTER(McQueryResult)]
    lib.mc_query_result_free.restype = None
    lib.mc_impute.argtypes = [OP, DP, MP, C.c_void_p, C.POINTER(McImputeResult)]
    lib.mc_impute_n_real.argtypes = [DP, C.c_void_p]
    lib.mc_divergence.argtypes = [OP, DP, MP, C.POINTER(McDivergenceResult)]
    lib.mc_divergence_result_free.argtypes = [C.POINTER(McDivergenceResult)]
    lib.mc_divergence_result_free.restype = None
    lib.mc_divergence_weights.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.mc_divergence_weights.restype = None
    lib.mc_divergence_tables.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 5
    lib.mc_divergence_tables.restype = None
    lib.mc_divergence_summary.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_int)] + [C.POINTER(C.c_double)] * 3
    lib.mc_divergence_summary.restype = None
    lib.mc_residual_correlation.argtypes = [DP, MP, C.POINTER(McResidResult)]
    lib.mc_resid_result_free.argtypes = [C.POINTER(McResidResult)]
    lib.mc_resid_result_free.restype = None
    lib.mc_residual_ratios.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mc_residual_ratios.restype = None
    lib.mc_residual_summary.argtypes = [C.c_int, C.c_void_p, C.POINTER(McResidResult)]
    lib.mc_residual_summary.restype = None
    lib.mc_read_structure.argtypes = [C.POINTER(CliOptionsAll), C.POINTER(CliDataAll)]
    lib.mc_read_bed.argtypes = [C.POINTER(CliOptionsAll), C.POINTER(CliDataAll)]
    lib.mc_free_data.argtypes = [C.POINTER(CliDataAll)]
    lib.mc_write_filled_structure.argtypes = [C.POINTER(CliOptionsAll), C.POINTER(CliDataAll), C.c_void_p, C.c_char_p]
    lib.mc_write_filled_bed.argtypes = [C.POINTER(CliOptionsAll), C.POINTER(CliDataAll), C.c_void_p, C.c_char_p]
    lib.mc_aic.restype = C.c_double
    lib.mc_aic.argtypes = [C.c_double, C.c_int]
    lib.mc_bic.restype = C.c_double
    lib.mc_bic.argtypes = [C.c_double, C.c_int, C.c_int]
    _lib = lib
    return lib


class Fit:
    """options + data + model triple, the argument convention of the reference's EM layer."""

    def __init__(self, ua, geno, K, device=0, **opts):
        self.lib = load()
        self.ua = np.ascontiguousarray(ua, dtype=np.int32)
        self.geno = np.ascontiguousarray(geno, dtype=np.uint8)
        I, L, p = self.geno.shape
        self.opt = McOptions()
        self.lib.mc_make_options(C.byref(self.opt))
        for k, v in opts.items():
            setattr(self.opt, k, v)
        self.dat = McData(I, L, p, self.ua.ctypes.data, self.geno.ctypes.data)
        if self.lib.mc_synchronize(C.byref(self.opt), C.byref(self.dat)):
            raise hip.HipError("mc_synchronize failed")
        self.mp = C.POINTER(McModel)()
        rc = self.lib.mc_model_create(C.byref(self.mp), C.byref(self.opt), C.byref(self.dat), K, device)
        if rc:
            raise hip.HipError("mc_model_create failed with status %d (no GPU => no product path)" % rc)
        self.K, self.I, self.T = K, I, int(self.ua.sum())
        self.indiv_q = bool(self.opt.admixture and not self.opt.eta_constrained)

    mod = property(lambda s: s.mp.contents)

    def close(self):
        if self.mp:
            self.lib.mc_model_free(self.mp)
            self.mp = C.POINTER(McModel)()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _a(self):
        return C.byref(self.opt), C.byref(self.dat), self.mp

    def set_params(self, q, p, slot=0):
        q = np.ascontiguousarray(q, dtype=np.float64)
        p = np.ascontiguousarray(p, dtype=np.float64)
        assert not self.lib.mc_model_set_q(self.mp, slot, q.ctypes.data)
        assert not self.lib.mc_model_set_p(self.mp, slot, p.ctypes.data)

    def get_q(self, slot):
        q = np.empty((self.I, self.K) if self.indiv_q else (self.K,))
        assert not self.lib.mc_model_get_q(self.mp, slot, q.ctypes.data)
        return q

    def get_p(self, slot):
        p = np.empty((self.K, self.T))
        assert not self.lib.mc_model_get_p(self.mp, slot, p.ctypes.data)
        return p

    def expected_counts(self):
        s = np.empty((self.I, self.K))
        assert not self.lib.mc_model_get_expected_counts(self.mp, s.ctypes.data)
        return s

    def reset(self):
        self.lib.mc_reset_model_state(self.mp)

    def initialize(self, seed):
        rng = McRng()
        self.lib.mc_srand(C.byref(rng), seed)
        rc = self.lib.mc_initialize_model(C.byref(self.opt), C.byref(self.dat), self.mp, C.byref(rng))
        if rc:
            raise hip.HipError("mc_initialize_model failed (%d)" % rc)
        return rng

    def em(self):
        self.lib.mc_em(*self._a())

    def em_step(self):
        return self.lib.mc_em_step(*self._a())

    def em_e_step(self):
        return self.lib.mc_em_e_step(*self._a())

    def accelerated_em_step(self):
        return self.lib.mc_accelerated_em_step(*self._a())

    def fit_unit(self, seed, unit):
        """initialisation `unit` of the run seeded with `seed` (stream jumped to the serial program's offset) + em()"""
        r = McUnitResult()
        rc = self.lib.mc_fit_unit(C.byref(self.opt), C.byref(self.dat), self.mp, seed, unit, C.byref(r))
        if rc:
            raise hip.HipError("mc_fit_unit failed (%d)" % rc)
        return r

    def no_parameters(self):
        return self.lib.mc_no_parameters(C.byref(self.opt), C.byref(self.dat), self.K)

    def log_likelihood(self, which):
        return self.lib.mc_log_likelihood(C.byref(self.opt), C.byref(self.dat), self.mp, which)

    def cross_validate(self, n_folds, floor=0.0):
        """mc_cross_validate on the estimate in slot mod.pindex: (cv, sum_log, n_copies, n_floored, per-fold list of
        (sum_log, n_copies, n_floored, EM iterations)); cv is NaN when a fold's fit stopped on NaN or a decrease.  floor <= 0:
        the default 1 / (I ploidy + 1).  Leaves the model as it found it."""
        r = McCvResult()
        rc = self.lib.mc_cross_validate(C.byref(self.opt), C.byref(self.dat), self.mp, n_folds, floor, C.byref(r))
        if rc:
            raise hip.HipError("mc_cross_validate failed (%d)" % rc)
        folds = [(r.fold_sum_log[f], r.fold_copies[f], r.fold_floored[f], r.fold_iter[f]) for f in range(n_folds)]
        return r.cv, r.sum_log, r.n_copies, r.n_floored, folds

    def locus_bootstrap(self, n_replicates, block=1):
        """mc_locus_bootstrap on the estimate in slot mod.pindex: (mean, se, count, result) -- mean and standard error of every
        entry of Q over the replicates (loci, or blocks of `block` neighbouring loci, drawn with replacement; each replicate fitted
        from the estimate), the number of replicates each entry was observed in, and the mc_se_result.  Leaves the model as it
        found it."""
        shape = (self.I, self.K) if self.indiv_q else (self.K,)
        mean, se, count = np.empty(shape), np.empty(shape), np.empty(shape, dtype=np.int32)
        r = McSeResult()
        rc = self.lib.mc_locus_bootstrap(C.byref(self.opt), C.byref(self.dat), self.mp, n_replicates, block, mean.ctypes.data,
                                         se.ctypes.data, count.ctypes.data, C.byref(r))
        if rc:
            raise hip.HipError("mc_locus_bootstrap failed (%d)" % rc)
        return mean, se, count, r

    def hide_queries(self, mask):
        """mc_query_hide: the individuals with mask[i] != 0 become individuals without an observed copy for every fit that
        follows (the device keeps their genotypes); call it right after the model is created, as the command line does"""
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        assert m.shape == (self.I,)
        rc = self.lib.mc_query_hide(self.mp, C.byref(self.dat), m.ctypes.data)
        if rc:
            raise hip.HipError("mc_query_hide failed (%d)" % rc)
        self._query_mask = m

    def fit_queries(self, mask=None):
        """mc_query_fit on the estimate in slot mod.pindex: dict with rows, q [n][K], logL, iter, converged (one entry per query
        individual in data order) and n_converged, n_failed, max_iter, sum_logL.  mask: the one hide_queries was given."""
        m = self._query_mask if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        r = McQueryResult()
        rc = self.lib.mc_query_fit(C.byref(self.opt), C.byref(self.dat), self.mp, m.ctypes.data, C.byref(r))
        if rc:
            raise hip.HipError("mc_query_fit failed (%d)" % rc)
        n, K = r.n, r.K
        out = dict(rows=np.ctypeslib.as_array(r.rows, shape=(n,)).copy(), q=np.ctypeslib.as_array(r.q, shape=(n, K)).copy(),
                   logL=np.ctypeslib.as_array(r.logL, shape=(n,)).copy(), iter=np.ctypeslib.as_array(r.iter, shape=(n,)).copy(),
                   converged=np.ctypeslib.as_array(r.converged, shape=(n,)).copy(), n_converged=r.n_converged,
                   n_failed=r.n_failed, max_iter=r.max_iter, sum_logL=r.sum_logL)
        self.lib.mc_query_result_free(C.byref(r))
        return out

    def impute(self):
        """mc_impute on the estimate in slot mod.pindex: (geno [I][L][ploidy] with the missing copies of the data set installed on
        the device filled in, dict with n_filled, n_left (copies), n_genotypes, sum_conf, mean_conf).  Leaves the model as it found
        it."""
        g = np.empty(self.geno.shape, dtype=np.uint8)
        r = McImputeResult()
        rc = self.lib.mc_impute(C.byref(self.opt), C.byref(self.dat), self.mp, g.ctypes.data, C.byref(r))
        if rc:
            raise hip.HipError("mc_impute failed (%d)" % rc)
        return g, dict(n_filled=r.n_filled, n_left=r.n_left, n_genotypes=r.n_genotypes, sum_conf=r.sum_conf, mean_conf=r.mean_conf)

    def divergence(self):
        """mc_divergence on the estimate in slot mod.pindex: dict with w, H [K], D, F [K][K], locus_ht, locus_f [L], n_loci, n_pairs,
        f_mean, f_min, f_max, sum_v, sum_ht, f_all (multiclust_amd/host/mc_host.h).  Leaves the model as it found it."""
        r = McDivergenceResult()
        rc = self.lib.mc_divergence(C.byref(self.opt), C.byref(self.dat), self.mp, C.byref(r))
        if rc:
            raise hip.HipError("mc_divergence failed (%d)" % rc)
        K, L = r.K, r.L
        out = dict(w=np.ctypeslib.as_array(r.w, shape=(K,)).copy(), H=np.ctypeslib.as_array(r.H, shape=(K,)).copy(),
                   D=np.ctypeslib.as_array(r.D, shape=(K, K)).copy(), F=np.ctypeslib.as_array(r.F, shape=(K, K)).copy(),
                   locus_ht=np.ctypeslib.as_array(r.locus_ht, shape=(L,)).copy(),
                   locus_f=np.ctypeslib.as_array(r.locus_f, shape=(L,)).copy(), n_loci=r.n_loci, n_pairs=r.n_pairs,
                   f_mean=r.f_mean, f_min=r.f_min, f_max=r.f_max, sum_v=r.sum_v, sum_ht=r.sum_ht, f_all=r.f_all)
        self.lib.mc_divergence_result_free(C.byref(r))
        return out

    def residual_correlation(self):
        """mc_residual_correlation on the estimate in slot mod.pindex: dict with cor [I][I], ind_mean, ind_max, ind_partner [I],
        n_pairs, mean, mean_abs, max, max_pair (multiclust_amd/host/mc_host.h).  Leaves the model as it found it."""
        r = McResidResult()
        rc = self.lib.mc_residual_correlation(C.byref(self.dat), self.mp, C.byref(r))
        if rc:
            raise hip.HipError("mc_residual_correlation failed (%d)" % rc)
        out = _resid_dict(r)
        self.lib.mc_resid_result_free(C.byref(r))
        return out

    def locus_lists(self, n_replicates, block=1):
        """the locus lists mc_locus_bootstrap installs for these arguments and the options' seed, one int32 array per replicate"""
        L = self.dat.L
        cap = self.lib.mc_se_list_capacity(L, block)
        if not cap or n_replicates < 0:
            raise hip.HipError("locus_lists: block must be in [1, L]")
        rng = McRng()
        self.lib.mc_srand(C.byref(rng), self.opt.seed)
        src, n = np.empty((max(n_replicates, 1), cap), dtype=np.int32), np.empty(max(n_replicates, 1), dtype=np.int32)
        if self.lib.mc_se_draw_lists(C.byref(rng), L, block, n_replicates, src.ctypes.data, n.ctypes.data):
            raise hip.HipError("mc_se_draw_lists failed")
        return [src[r, :n[r]].copy() for r in range(n_replicates)]
