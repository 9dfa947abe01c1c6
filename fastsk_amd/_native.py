"""ctypes view of the C ABI in ``include/fastsk_amd.h`` (``libfastsk_amd.so``).

Used by the staged / multi-GPU host code (``fastsk_amd.distributed``), ``bench.py`` and the parity
tests; the drop-in ``FastSK`` class itself is the pybind11 module ``fastsk_amd._fastsk`` built on
the same library. There is no CPU fallback: if the HIP library is missing this module raises.
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libfastsk_amd.so")

PATH_AUTO, PATH_DENSE, PATH_SPARSE = 0, 1, 2
COLL_AUTO, COLL_RCCL, COLL_P2P = 0, 1, 2
ABI_VERSION = 5

ERRORS = {-1: "FSK_EINVAL", -2: "FSK_ESHORT", -3: "FSK_ESTATE", -4: "FSK_EDEVICE", -5: "FSK_ENOMEM",
          -6: "FSK_EUNSUPPORTED"}


class FskError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (ERRORS.get(code, "FSK_E?"), code, msg))
        self.code = code


class Config(C.Structure):
    _fields_ = [("g", C.c_int32), ("m", C.c_int32), ("t", C.c_int32), ("approx", C.c_int32),
                ("delta", C.c_double), ("max_iters", C.c_int32), ("skip_variance", C.c_int32),
                ("device", C.c_int32), ("path", C.c_int32), ("profile", C.c_int32),
                ("skip_test_block", C.c_int32), ("collective", C.c_int32), ("bands", C.c_int32),
                ("deadline_ms", C.c_int32), ("reserved", C.c_int32 * 1)]


class Stats(C.Structure):
    _fields_ = [("n_seq", C.c_int64), ("n_train", C.c_int64), ("n_test", C.c_int64), ("n_feat", C.c_int64),
                ("n_pairs", C.c_int64), ("alphabet", C.c_int32), ("bits_per_symbol", C.c_int32),
                ("key_space", C.c_int64), ("path_used", C.c_int32), ("n_combos_total", C.c_int32),
                ("combos_done", C.c_int64), ("cell_updates", C.c_uint64), ("sort_records", C.c_uint64),
                ("sort_passes", C.c_int32), ("launches", C.c_int32), ("ms_count", C.c_double),
                ("ms_tile", C.c_double), ("ms_extract", C.c_double), ("ms_sort", C.c_double),
                ("ms_segment", C.c_double), ("ms_pairs", C.c_double), ("ms_total", C.c_double),
                ("n_tile_launches", C.c_int64), ("dense_macs", C.c_uint64), ("panel_bytes", C.c_uint64),
                ("u4_tile_launches", C.c_double), ("max_windows", C.c_double), ("count_launches", C.c_double),
                ("compact_keys_avg", C.c_double), ("batches_redone", C.c_double), ("combos_issued", C.c_double),
                ("sparse_form", C.c_double), ("sparse_passes", C.c_double), ("share_positions", C.c_double), ("share_groups", C.c_double),
                ("sparse_desc", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class SvmInfo(C.Structure):
    _fields_ = [("iterations", C.c_int64), ("gap", C.c_double), ("objective", C.c_double), ("n_sv", C.c_int64),
                ("n_bsv", C.c_int64), ("converged", C.c_int32), ("form", C.c_int32), ("launches", C.c_int64),
                ("ms", C.c_double), ("reserved", C.c_double * 4)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        d["converged"] = bool(d["converged"])
        d["form"] = _FORMS.get(d["form"], "none")
        return d


_FORMS = {1: "workgroup", 2: "two-launch"}

SVM_KERNEL_RESULT, SVM_KERNEL_ROWS = 0, 1   # fsk_svm_set_kernel
_SVM_KERNELS = {"fastsk": SVM_KERNEL_RESULT, "result": SVM_KERNEL_RESULT, "linear": SVM_KERNEL_ROWS, "rows": SVM_KERNEL_ROWS}


class RowsInfo(C.Structure):
    _fields_ = [("n_train", C.c_int64), ("n_seq", C.c_int64), ("tile", C.c_int32), ("panel", C.c_int32), ("tiles", C.c_int64),
                ("builds", C.c_int64), ("scratch_bytes", C.c_int64), ("resident_bytes", C.c_int64), ("ms_scratch", C.c_double),
                ("ms_product", C.c_double), ("reserved", C.c_double * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class SvmCvProblem(C.Structure):
    _fields_ = [("n_rows", C.c_int64), ("iterations", C.c_int64), ("gap", C.c_double), ("objective", C.c_double),
                ("rho", C.c_double), ("C", C.c_double), ("n_sv", C.c_int64), ("n_bsv", C.c_int64), ("converged", C.c_int32),
                ("fold", C.c_int32), ("reserved", C.c_double * 2)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        d["converged"] = bool(d["converged"])
        return d


class SvmCvScore(C.Structure):
    _fields_ = [("C", C.c_double), ("auc", C.c_double), ("accuracy", C.c_double), ("reserved", C.c_double)]


class SvmCvInfo(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_folds", C.c_int32), ("n_C", C.c_int32), ("form", C.c_int32), ("reserved0", C.c_int32),
                ("launches", C.c_int64), ("ms", C.c_double), ("reserved", C.c_double * 4)]


class SvrCvScore(C.Structure):
    _fields_ = [("C", C.c_double), ("epsilon", C.c_double), ("mse", C.c_double), ("mae", C.c_double), ("r2", C.c_double),
                ("r", C.c_double), ("reserved", C.c_double * 2)]


class SvmMulticlassPair(C.Structure):
    _fields_ = [("class_a", C.c_int32), ("class_b", C.c_int32), ("n_rows", C.c_int64), ("iterations", C.c_int64),
                ("gap", C.c_double), ("objective", C.c_double), ("rho", C.c_double), ("n_sv", C.c_int64), ("n_bsv", C.c_int64),
                ("converged", C.c_int32), ("reserved0", C.c_int32), ("reserved", C.c_double * 2)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}
        d["converged"] = bool(d["converged"])
        return d


class SvmMulticlassInfo(C.Structure):
    _fields_ = [("k", C.c_int32), ("n_pairs", C.c_int32), ("form", C.c_int32), ("reserved0", C.c_int32), ("launches", C.c_int64),
                ("n_sv", C.c_int64), ("n_alpha", C.c_int64), ("ms", C.c_double), ("reserved", C.c_double * 4)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}
        d["form"] = _FORMS.get(d["form"], "none")
        return d


class SvmPlattInfo(C.Structure):
    _fields_ = [("A", C.c_double), ("B", C.c_double), ("iterations", C.c_int32), ("status", C.c_int32), ("n_folds", C.c_int32),
                ("form", C.c_int32), ("launches", C.c_int64), ("ms", C.c_double), ("reserved", C.c_double * 4)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        d["form"] = _FORMS.get(d["form"], "none")
        return d


class MultiInfo(C.Structure):
    _fields_ = [("ndev", C.c_int32), ("devices", C.c_int32 * 16), ("collective", C.c_int32), ("comm_ranks", C.c_int32),
                ("bands", C.c_int32), ("narrow", C.c_int32), ("reduce_bytes", C.c_int64),
                ("combos_per_engine", C.c_int64 * 16), ("reserved", C.c_double * 4)]

    def as_dict(self):
        n = self.ndev
        return {"ndev": n, "devices": list(self.devices[:n]),
                "collective": {COLL_RCCL: "rccl", COLL_P2P: "p2p"}.get(self.collective, "none"),
                "comm_ranks": self.comm_ranks, "bands": self.bands, "narrow": bool(self.narrow),
                "reduce_bytes": self.reduce_bytes, "combos_per_engine": list(self.combos_per_engine[:n])}


# every symbol include/fastsk_amd.h declares (checked by tests/test_abi.py)
SYMBOLS = ["fsk_create", "fsk_destroy", "fsk_last_error", "fsk_abi_version", "fsk_device_count", "fsk_compute",
           "fsk_set_combo_order", "fsk_set_seed", "fsk_load_sequences", "fsk_bind_counts",
           "fsk_counts_device_ptr", "fsk_reset_counts", "fsk_reset_counts_rows", "fsk_accumulate", "fsk_accumulate_rows", "fsk_synchronize", "fsk_finalize",
           "fsk_get_block", "fsk_get_block_device", "fsk_get_train", "fsk_get_test", "fsk_get_triangle", "fsk_get_counts",
           "fsk_get_counts_block", "fsk_get_counts_cells", "fsk_get_stdevs", "fsk_save_kernel", "fsk_get_stats", "fsk_num_combos",
           "fsk_combo_positions", "fsk_stream_wait_engine", "fsk_engine_wait_stream", "fsk_read_fasta", "fsk_sequential_sum",
           "fsk_run_chains", "fsk_get_kernel_sum_device", "fsk_set_kernel_sum_device", "fsk_create_multi", "fsk_get_multi_info",
           "fsk_counts_digest", "fsk_alloc_block_device", "fsk_free_device", "fsk_set_skip_test_block",
           "fsk_get_triangle_device", "fsk_alloc_triangle_device", "fsk_set_tuning", "fsk_get_tuning", "fsk_tuning_keys", "fsk_seed_order",
           "fsk_set_complement", "fsk_set_mismatch_weights", "fsk_get_mismatch_info", "fsk_get_mismatch_times", "fsk_mismatch_levels",
           "fsk_set_wildcards", "fsk_set_center_weights", "fsk_svm_train", "fsk_svm_get_model", "fsk_svm_decision",
           "fsk_svm_decision_device", "fsk_svm_cv", "fsk_svm_cv_get", "fsk_svm_cv_get_alpha", "fsk_rows_build", "fsk_rows_get_block",
           "fsk_rows_get_block_device", "fsk_rows_get_info", "fsk_svm_set_kernel", "fsk_svm_get_kernel",
           "fsk_svm_set_class_weights", "fsk_svm_get_class_weights", "fsk_svm_platt_fit", "fsk_svm_calibrate",
           "fsk_svm_get_calibration", "fsk_svm_proba", "fsk_svr_train", "fsk_svr_get_model", "fsk_svr_cv", "fsk_svr_cv_get",
           "fsk_svm_train_multiclass", "fsk_svm_multiclass_get_model", "fsk_svm_multiclass_decision",
           "fsk_svm_multiclass_decision_device", "fsk_svm_multiclass_cv", "fsk_svm_multiclass_cv_get",
           "fsk_svm_multiclass_calibrate", "fsk_svm_multiclass_get_calibration", "fsk_svm_multiclass_set_calibration",
           "fsk_svm_multiclass_proba", "fsk_svm_multiclass_proba_device", "fsk_exp_neg"]


_hip_shared = False


def _mapped_runtimes():
    """Paths of the libamdhip64 / libhsa-runtime64 images mapped into this process."""
    found = {}
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                path = line.rsplit(None, 1)[-1]
                base = os.path.basename(path)
                for stem in ("libamdhip64.so", "libhsa-runtime64.so"):
                    if base.startswith(stem):
                        found.setdefault(stem, set()).add(path)
    except OSError:
        pass
    return found


def share_hip_runtime_with_torch():
    """One HIP runtime per process. A PyTorch-ROCm wheel carries its own libamdhip64 /
    libhsa-runtime64; if this engine binds /opt/rocm's copy first and torch is imported later, the
    process ends up with two HSA runtimes and the second one to initialise finds no GPU. So when
    torch is installed but not imported yet, and no HIP runtime is mapped yet (a profiler's preload, an
    earlier import), its copies (same SONAMEs) are loaded first and the engine binds to them —
    exactly what happens anyway when torch is imported before this package.
    No torch installed: nothing to do, /opt/rocm's runtime is used."""
    global _hip_shared
    if _hip_shared or "torch" in sys.modules:
        _hip_shared = True
        return
    _hip_shared = True
    if _mapped_runtimes():
        return  # a runtime is already in the process: loading torch's copy by path would add a second image
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
        for name in ("libhsa-runtime64.so", "libamdhip64.so"):
            path = os.path.join(libdir, name)
            if os.path.exists(path):
                C.CDLL(path, mode=C.RTLD_GLOBAL)
    except OSError:
        pass


def check_single_hip_runtime():
    """Warn when two different libamdhip64 images ended up in the process (e.g. a torch wheel built
    against another ROCm major: different SONAME, so the preload above cannot unify them)."""
    images = _mapped_runtimes().get("libamdhip64.so", set())
    real = {os.path.realpath(p) for p in images}
    if len(real) > 1:
        import warnings
        warnings.warn("two HIP runtimes are mapped into this process (%s): the engine and torch will not see the same "
                      "GPU state; import torch before fastsk_amd, or use a torch wheel built for this ROCm" % ", ".join(sorted(real)))


class Library:
    """The loaded shared library with typed entry points."""

    def __init__(self, path=None, optional=()):
        """``optional``: symbols that an older build of the library may lack (tools that load such a build beside this one);
        they are left unbound, every other symbol must be there."""
        if path is None:
            share_hip_runtime_with_torch()  # the product library; an explicit path is the CPU emulation of the tests
        path = path or LIB_PATH
        if not os.path.exists(path):
            raise ImportError(
                "%s not found: build the HIP engine first (python -c 'import __graft_entry__ as g; g.build()'). "
                "fastsk_amd has no CPU fallback." % path)
        L = C.CDLL(path)
        if path == LIB_PATH:
            check_single_hip_runtime()
        self.path = path
        L.fsk_abi_version.restype = C.c_int
        if L.fsk_abi_version() != ABI_VERSION:  # a stale build: its structs and symbols are not the ones bound below
            raise ImportError("%s speaks ABI version %d, this package needs %d: rebuild it (python -c 'import __graft_entry__ "
                              "as g; g.build()')" % (path, L.fsk_abi_version(), ABI_VERSION))
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        sig = {
            "fsk_create": ([C.POINTER(Config), C.POINTER(vp)], C.c_int),
            "fsk_destroy": ([vp], None),
            "fsk_last_error": ([vp], C.c_char_p),
            "fsk_abi_version": ([], C.c_int),
            "fsk_device_count": ([], C.c_int),
            "fsk_compute": ([vp, vp, vp, i64, i64], C.c_int),
            "fsk_set_combo_order": ([vp, vp, i32], C.c_int),
            "fsk_set_seed": ([vp, C.c_uint64], C.c_int),
            "fsk_load_sequences": ([vp, vp, vp, i64, i64], C.c_int),
            "fsk_bind_counts": ([vp, vp, i64], C.c_int),
            "fsk_counts_device_ptr": ([vp, C.POINTER(vp)], C.c_int),
            "fsk_reset_counts": ([vp], C.c_int),
            "fsk_reset_counts_rows": ([vp, i64, i64], C.c_int),
            "fsk_accumulate": ([vp, vp, i32], C.c_int),
            "fsk_accumulate_rows": ([vp, vp, i32, i64, i64], C.c_int),
            "fsk_synchronize": ([vp], C.c_int),
            "fsk_finalize": ([vp], C.c_int),
            "fsk_get_block": ([vp, i64, i64, i64, i64, vp], C.c_int),
            "fsk_get_block_device": ([vp, i64, i64, i64, i64, vp], C.c_int),
            "fsk_get_train": ([vp, vp], C.c_int),
            "fsk_get_test": ([vp, vp], C.c_int),
            "fsk_get_triangle": ([vp, vp], C.c_int),
            "fsk_get_counts": ([vp, vp], C.c_int),
            "fsk_get_counts_block": ([vp, i64, i64, i64, i64, vp], C.c_int),
            "fsk_get_counts_cells": ([vp, vp, vp, i64, vp], C.c_int),
            "fsk_stream_wait_engine": ([vp, vp], C.c_int),
            "fsk_engine_wait_stream": ([vp, vp], C.c_int),
            "fsk_read_fasta": ([C.c_char_p, vp, C.POINTER(i32), vp, i64, vp, vp, i64, C.POINTER(i64), C.POINTER(i64), C.c_char_p, i32], C.c_int),
            "fsk_sequential_sum": ([vp, vp, i64, C.POINTER(C.c_double)], C.c_int),
            "fsk_run_chains": ([vp, i32, i32], C.c_int),
            "fsk_get_kernel_sum_device": ([vp, vp], C.c_int),
            "fsk_set_kernel_sum_device": ([vp, vp], C.c_int),
            "fsk_get_stdevs": ([vp, vp, i32, C.POINTER(i32)], C.c_int),
            "fsk_save_kernel": ([vp, C.c_char_p], C.c_int),
            "fsk_get_stats": ([vp, C.POINTER(Stats)], C.c_int),
            "fsk_num_combos": ([i32, i32], i64),
            "fsk_combo_positions": ([i32, i32, i64, vp], C.c_int),
            "fsk_create_multi": ([C.POINTER(Config), vp, i32, C.POINTER(vp)], C.c_int),
            "fsk_get_multi_info": ([vp, C.POINTER(MultiInfo)], C.c_int),
            "fsk_counts_digest": ([vp, i64, i64, vp], C.c_int),
            "fsk_alloc_block_device": ([vp, i64, i64, i64, i64, C.POINTER(vp)], C.c_int),
            "fsk_free_device": ([vp, vp], C.c_int),
            "fsk_set_skip_test_block": ([vp, i32], C.c_int),
            "fsk_get_triangle_device": ([vp, vp], C.c_int),
            "fsk_alloc_triangle_device": ([vp, C.POINTER(vp)], C.c_int),
            "fsk_set_tuning": ([vp, C.c_char_p, i64], C.c_int),
            "fsk_get_tuning": ([vp, C.c_char_p, C.POINTER(i64)], C.c_int),
            "fsk_tuning_keys": ([], C.c_char_p),
            "fsk_seed_order": ([C.c_uint64, i64, vp], C.c_int),
            "fsk_set_complement": ([vp, vp, vp, i32], C.c_int),
            "fsk_set_wildcards": ([vp, vp, i32], C.c_int),
            "fsk_set_center_weights": ([vp, vp, i32], C.c_int),
            "fsk_set_mismatch_weights": ([vp, vp, i32], C.c_int),
            "fsk_get_mismatch_info": ([vp, C.POINTER(i32), vp, vp, i32], C.c_int),
            "fsk_get_mismatch_times": ([vp, vp, vp, i32], C.c_int),
            "fsk_mismatch_levels": ([i32, vp, i32, vp, C.POINTER(i32)], C.c_int),
            "fsk_svm_train": ([vp, vp, i64, C.c_double, C.c_double, i64], C.c_int),
            "fsk_svm_get_model": ([vp, vp, C.POINTER(C.c_double), C.POINTER(SvmInfo)], C.c_int),
            "fsk_svm_decision": ([vp, i64, i64, vp], C.c_int),
            "fsk_svm_decision_device": ([vp, i64, i64, vp], C.c_int),
            "fsk_svm_cv": ([vp, vp, i64, vp, i32, vp, i32, C.c_double, i64], C.c_int),
            "fsk_svm_cv_get": ([vp, vp, vp, vp, C.POINTER(SvmCvInfo)], C.c_int),
            "fsk_svm_cv_get_alpha": ([vp, i32, vp], C.c_int),
            "fsk_rows_build": ([vp], C.c_int),
            "fsk_rows_get_block": ([vp, i64, i64, i64, i64, i32, vp], C.c_int),
            "fsk_rows_get_block_device": ([vp, i64, i64, i64, i64, i32, vp], C.c_int),
            "fsk_rows_get_info": ([vp, C.POINTER(RowsInfo)], C.c_int),
            "fsk_svm_set_kernel": ([vp, i32], C.c_int),
            "fsk_svm_get_kernel": ([vp, C.POINTER(i32)], C.c_int),
            "fsk_svm_set_class_weights": ([vp, C.c_double, C.c_double], C.c_int),
            "fsk_svm_get_class_weights": ([vp, C.POINTER(C.c_double), C.POINTER(C.c_double)], C.c_int),
            "fsk_svm_platt_fit": ([vp, vp, i64, C.POINTER(SvmPlattInfo)], C.c_int),
            "fsk_svm_calibrate": ([vp, vp, i32], C.c_int),
            "fsk_svm_get_calibration": ([vp, vp, C.POINTER(SvmPlattInfo)], C.c_int),
            "fsk_svm_proba": ([vp, i64, i64, vp], C.c_int),
            "fsk_svr_train": ([vp, vp, i64, C.c_double, C.c_double, C.c_double, i64], C.c_int),
            "fsk_svr_get_model": ([vp, vp, vp, C.POINTER(C.c_double), C.POINTER(SvmInfo)], C.c_int),
            "fsk_svr_cv": ([vp, vp, i64, vp, i32, vp, i32, vp, i32, C.c_double, i64], C.c_int),
            "fsk_svr_cv_get": ([vp, vp, vp, vp, C.POINTER(SvmCvInfo)], C.c_int),
            "fsk_svm_train_multiclass": ([vp, vp, i64, C.c_double, vp, C.c_double, i64], C.c_int),
            "fsk_svm_multiclass_get_model": ([vp, vp, vp, vp, C.POINTER(SvmMulticlassInfo)], C.c_int),
            "fsk_svm_multiclass_decision": ([vp, i64, i64, vp, vp], C.c_int),
            "fsk_svm_multiclass_decision_device": ([vp, i64, i64, vp, vp], C.c_int),
            "fsk_svm_multiclass_cv": ([vp, vp, i64, vp, i32, vp, i32, vp, C.c_double, i64], C.c_int),
            "fsk_svm_multiclass_cv_get": ([vp, vp, vp, vp, C.POINTER(SvmCvInfo)], C.c_int),
            "fsk_svm_multiclass_calibrate": ([vp, vp, i32], C.c_int),
            "fsk_svm_multiclass_get_calibration": ([vp, vp, vp], C.c_int),
            "fsk_svm_multiclass_set_calibration": ([vp, vp, vp], C.c_int),
            "fsk_svm_multiclass_proba": ([vp, i64, i64, vp, vp, vp], C.c_int),
            "fsk_svm_multiclass_proba_device": ([vp, i64, i64, vp, vp, vp], C.c_int),
            "fsk_exp_neg": ([C.c_double], C.c_double),
        }
        for name, (argtypes, restype) in sig.items():
            if name in optional and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = restype
        self.L = L

    def num_combos(self, g, m):
        return int(self.L.fsk_num_combos(g, m))

    def combo_positions(self, g, k, combo):
        out = np.zeros(k, dtype=np.int32)
        rc = self.L.fsk_combo_positions(g, k, combo, out.ctypes.data)
        if rc:
            raise FskError(rc, "bad combination id")
        return out

    def seed_order(self, seed, n):
        """The combo order ``fsk_set_seed(seed)`` stands for: the reference's std::shuffle with time(0) == seed."""
        out = np.zeros(max(n, 1), dtype=np.int32)
        rc = self.L.fsk_seed_order(seed, n, out.ctypes.data)
        if rc:
            raise FskError(rc, "bad length")
        return out[:n]

    def device_count(self):
        return int(self.L.fsk_device_count())

    def mismatch_levels(self, g, weights):
        """``fsk_mismatch_levels``: the level coefficients a_0..a_d of the mismatch weights c_0..c_{n-1} at window length g."""
        c = np.ascontiguousarray([int(w) for w in weights], dtype=np.uint64)
        a = np.zeros(max(len(c), 1), dtype=np.int64)
        n = C.c_int32(0)
        rc = self.L.fsk_mismatch_levels(g, c.ctypes.data, len(c), a.ctypes.data, C.byref(n))
        if rc:
            raise FskError(rc, (self.L.fsk_last_error(None) or b"").decode())
        return [int(v) for v in a[:n.value]]

    def platt_fit(self, dec, labels):
        """``fsk_svm_platt_fit``: LIBSVM's sigmoid_train on decision values and labels in {-1, +1} (host only). Returns
        ``A``, ``B`` (P(y = +1 | f) = 1 / (1 + exp(A f + B))), ``iterations`` and ``status`` (0: the gradient fell below 1e-5;
        1: 100 iterations; 2: the line search failed)."""
        dec = np.ascontiguousarray(dec, dtype=np.float64)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if dec.ndim != 1 or labels.ndim != 1 or len(dec) != len(labels):
            raise ValueError("dec and labels must be 1-D and of one length")
        if len(dec) < 1:
            raise ValueError("platt_fit: at least one decision value")
        wrong = np.flatnonzero((labels != 1) & (labels != -1))
        if len(wrong):
            raise ValueError("platt_fit: label %d is %d: labels must be -1 or +1" % (wrong[0], labels[wrong[0]]))
        info = SvmPlattInfo()
        rc = self.L.fsk_svm_platt_fit(dec.ctypes.data if len(dec) else None, labels.ctypes.data if len(labels) else None, len(dec),
                                      C.byref(info))
        if rc:
            raise FskError(rc, "fsk_svm_platt_fit refused its arguments")
        return {"A": info.A, "B": info.B, "iterations": info.iterations, "status": info.status}

    def exp_neg(self, x):
        """``fsk_exp_neg``: exp(x) for x <= 0 as the fixed sequence of IEEE operations the probability kernel uses (host only)."""
        return float(self.L.fsk_exp_neg(float(x)))

    def tuning_keys(self):
        """{key: (default, lowest, highest, what it does)} — every knob fsk_set_tuning / FSK_TUNING takes."""
        out = {}
        for line in self.L.fsk_tuning_keys().decode().splitlines():
            head, rng, doc = line.split(" ", 2)
            key, default = head.split("=")
            lo, hi = rng.strip("[]").split("..")
            out[key] = (int(default), int(lo), int(hi), doc)
        return out


_default = None


def library():
    """The product library (hipcc build). Raises ImportError when it has not been built."""
    global _default
    if _default is None:
        _default = Library()
    return _default


def complement_arrays(mapping):
    """``{token_id: token_id}`` -> (tokens int32, complements int32) for ``fsk_set_complement``, checked as the engine
    checks it (an involution on its domain; self-pairs allowed): ``ValueError`` otherwise. ``None`` / ``False`` / an empty
    mapping: two empty arrays, i.e. the mode off."""
    if mapping is None or mapping is False:
        mapping = {}
    if not hasattr(mapping, "items"):
        raise ValueError("revcomp must be None, False or a mapping {token_id: token_id}")
    pairs = []
    for k, v in mapping.items():
        if isinstance(k, bool) or isinstance(v, bool) or int(k) != k or int(v) != v:
            raise ValueError("revcomp: token ids must be integers, got %r -> %r" % (k, v))
        if not (-2 ** 31 <= int(k) < 2 ** 31 and -2 ** 31 <= int(v) < 2 ** 31):
            raise ValueError("revcomp: token ids must fit 32 bits")
        pairs.append((int(k), int(v)))
    as_map = dict(pairs)
    if len(as_map) != len(pairs):
        raise ValueError("revcomp: a token is listed twice")
    for k, v in pairs:
        if v not in as_map:
            raise ValueError("revcomp: token %d maps to %d, which is not listed" % (k, v))
        if as_map[v] != k:
            raise ValueError("revcomp is not an involution: %d -> %d -> %d" % (k, v, as_map[v]))
    return (np.array([k for k, _ in pairs], dtype=np.int32), np.array([v for _, v in pairs], dtype=np.int32))


def wildcard_array(wildcards):
    """The ``wildcards=`` keyword -> int32 array for ``fsk_set_wildcards``, checked as the engine checks it (integers that
    fit 32 bits, none listed twice): ``ValueError`` otherwise. ``None`` / ``False`` / an empty sequence: an empty array, i.e.
    the mode off."""
    if wildcards is None or wildcards is False:
        return np.zeros(0, dtype=np.int32)
    if isinstance(wildcards, (str, bytes)) or not hasattr(wildcards, "__iter__"):
        raise ValueError("wildcards must be None or a sequence of token ids")
    out = []
    for t in wildcards:
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)):
            raise ValueError("wildcards: token ids must be integers, got %r" % (t,))
        if not -2 ** 31 <= int(t) < 2 ** 31:
            raise ValueError("wildcards: token ids must fit 32 bits")
        out.append(int(t))
    if len(set(out)) != len(out):
        raise ValueError("wildcards: a token is listed twice")
    return np.array(out, dtype=np.int32)


def center_weight_array(center_weights):
    """The ``center_weights=`` keyword -> uint32 array for ``fsk_set_center_weights``, checked as the engine checks it (at
    most 4096 integers in 0..255, the first at least 1): ``ValueError`` otherwise. ``None`` / ``False`` / an empty sequence:
    an empty array, i.e. the mode off."""
    if center_weights is None or center_weights is False:
        return np.zeros(0, dtype=np.uint32)
    if isinstance(center_weights, (str, bytes)) or not hasattr(center_weights, "__iter__"):
        raise ValueError("center_weights must be None or a sequence of integers")
    out = []
    for w in center_weights:
        if isinstance(w, bool) or not isinstance(w, (int, np.integer)):
            raise ValueError("center_weights: weights must be integers, got %r" % (w,))
        if not 0 <= int(w) <= 255:
            raise ValueError("center_weights: weights must lie in 0..255, got %d" % int(w))
        out.append(int(w))
    if len(out) > 4096:
        raise ValueError("center_weights: %d entries, at most 4096" % len(out))
    if out and out[0] == 0:
        raise ValueError("center_weights: the first entry (the centre's weight) must be at least 1")
    return np.array(out, dtype=np.uint32)


def stratified_folds(labels, k, seed=0):
    """Fold ids 0..k-1 for ``cross_validate_svm`` (host only), stratified by label: walk the rows in the order
    ``np.random.Generator(np.random.PCG64(seed)).permutation(n)``; the c-th row met of a class (c = 0, 1, ...) gets fold
    ``c % k``. Every fold so holds its share of each class to within one row. -> int32 array [n]."""
    labels = np.asarray(labels)
    if labels.ndim != 1:
        raise ValueError("stratified_folds: labels must be 1-D")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 2:
        raise ValueError("stratified_folds: k must be an integer of at least 2")
    fold = np.zeros(len(labels), dtype=np.int32)
    met = {}
    for t in np.random.Generator(np.random.PCG64(seed)).permutation(len(labels)).tolist():
        c = met.get(labels[t].item(), 0)
        fold[t] = c % k
        met[labels[t].item()] = c + 1
    return fold


def kfold(n, k, seed=0):
    """Fold ids 0..k-1 for ``cross_validate_svr`` (host only): the rows in the order
    ``np.random.Generator(np.random.PCG64(seed)).permutation(n)`` are dealt round-robin, the c-th row met gets fold ``c % k``.
    -> int32 array [n]."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
        raise ValueError("kfold: n must be a non-negative integer")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 2:
        raise ValueError("kfold: k must be an integer of at least 2")
    fold = np.zeros(int(n), dtype=np.int32)
    fold[np.random.Generator(np.random.PCG64(seed)).permutation(int(n))] = np.arange(int(n), dtype=np.int32) % np.int32(k)
    return fold


def class_weights(labels, spec):
    """The ``class_weight=`` keyword -> ``(w_pos, w_neg)`` for ``fsk_svm_set_class_weights`` (host only). ``None``: (1, 1).
    ``"balanced"``: ``n / (2 n_pos)``, ``n / (2 n_neg)`` as scikit-learn's, computed ONCE from all training labels: the folds
    of a cross-validation or a calibration solve with these same two weights, they are not recomputed per fold. A pair
    ``(w_pos, w_neg)``, or a dict keyed by 1 and -1 (a missing key is 1). ``ValueError`` unless both are positive finite
    numbers."""
    if spec is None:
        return 1.0, 1.0
    if isinstance(spec, str):
        if spec != "balanced":
            raise ValueError("class_weight %r: None, \"balanced\", a pair (w_pos, w_neg) or a dict keyed by 1 / -1" % (spec,))
        labels = np.asarray(labels)
        n, n_pos = len(labels), int((labels > 0).sum())
        if n_pos == 0 or n_pos == n:
            raise ValueError("class_weight=\"balanced\": only one class is present")
        w = (n / (2.0 * n_pos), n / (2.0 * (n - n_pos)))
    elif hasattr(spec, "items"):
        if not set(spec) <= {1, -1}:
            raise ValueError("class_weight: a dict is keyed by 1 and -1")
        w = (spec.get(1, 1.0), spec.get(-1, 1.0))
    else:
        w = tuple(spec)
        if len(w) != 2:
            raise ValueError("class_weight: a pair (w_pos, w_neg)")
    w = (float(w[0]), float(w[1]))
    if not all(np.isfinite(x) and x > 0.0 for x in w):
        raise ValueError("class_weight: the weights must be positive finite numbers, got %r" % (w,))
    return w


def multiclass_weights(labels, spec):
    """The ``class_weight=`` keyword of ``fit_svm_multiclass`` -> one weight a class, in ascending class order (host only), or
    None. ``None``: None (every weight 1). ``"balanced"``: ``n / (k count_c)`` as scikit-learn's, computed ONCE from all
    training labels. A dict keyed by label (a missing class is 1; a key that is no class is a ``ValueError``). ``ValueError``
    unless every weight is a positive finite number."""
    if spec is None:
        return None
    classes, counts = np.unique(np.asarray(labels), return_counts=True)
    if isinstance(spec, str):
        if spec != "balanced":
            raise ValueError("class_weight %r: None, \"balanced\" or a dict keyed by label" % (spec,))
        w = [len(labels) / (float(len(classes)) * float(c)) for c in counts.tolist()]
    elif hasattr(spec, "items"):
        known = set(classes.tolist())
        for key in spec:
            if isinstance(key, bool) or not isinstance(key, (int, np.integer)) or int(key) not in known:
                raise ValueError("class_weight: %r is not a class of the labels" % (key,))
        w = [float({int(a): b for a, b in spec.items()}.get(c, 1.0)) for c in classes.tolist()]
    else:
        raise ValueError("class_weight: None, \"balanced\" or a dict keyed by label")
    if not all(np.isfinite(x) and x > 0.0 for x in w):
        raise ValueError("class_weight: the weights must be positive finite numbers, got %r" % (w,))
    return np.array(w, dtype=np.float64)


def center_profile(plateau, halflife, levels=8, floor=0):
    """A centre-weight profile for ``center_weights=`` (host only): ``levels`` within ``plateau`` windows of the centre,
    halved every ``halflife`` windows beyond, rounded to integers and never below ``floor`` --
    ``w[d] = max(floor, int(levels * 2 ** (-max(0, d - plateau) / halflife) + 0.5))`` -- cut where it first reaches its
    final constant (the last entry extends outwards). The shape of LS-GKM's ``-M`` / ``-H`` weighting, quantised; not its
    constants. ``ValueError`` when the arguments are out of range or the profile would be longer than 4096 entries."""
    for name, v in (("plateau", plateau), ("levels", levels), ("floor", floor)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("center_profile: %s must be an integer" % name)
    if plateau < 0 or not 1 <= levels <= 255 or not 0 <= floor <= 255:
        raise ValueError("center_profile: need plateau >= 0, 1 <= levels <= 255 and 0 <= floor <= 255")
    if not halflife > 0:
        raise ValueError("center_profile: halflife must be positive")
    final = max(int(floor), 0)  # (the weight decays to 0 before rounding: the final constant is the floor)
    out = []
    d = 0
    while True:
        w = max(int(floor), int(levels * 2.0 ** (-max(0, d - plateau) / float(halflife)) + 0.5))
        out.append(w)
        if w == final:
            break
        d += 1
        if d >= 4096:
            raise ValueError("center_profile: the profile reaches its final constant past 4096 entries")
    return out


def mismatch_levels(g, weights, lib=None):
    """The level coefficients ``a_0..a_d`` of mismatch weights ``c_0..c_m`` at window length ``g`` (``fsk_mismatch_levels``, host
    only): ``sum_h c_h N_h == sum_j a_j S_j`` with ``S_j`` the raw kernel of ``(g, m=j)``. ``d`` is the last ``h`` with
    ``c_h != 0``."""
    return (lib or library()).mismatch_levels(g, weights)


def solve_mismatch_levels(g, weights):
    """The same recurrence in Python integers (no library): a_d = c_d, a_h = c_h - sum_{j>h} a_j C(g-h, j-h)."""
    from math import comb
    c = [int(w) for w in weights]
    d = max(h for h, w in enumerate(c) if w) if any(c) else 0
    a = [0] * (d + 1)
    for h in range(d, -1, -1):
        a[h] = c[h] - sum(a[j] * comb(g - h, j - h) for j in range(h + 1, d + 1))
    return a


def mismatch_weights(g, m, weights=None, max_mismatches=None):
    """The ``weights=`` / ``max_mismatches=`` keywords checked and brought to one form: ``None`` (mode off) or the list
    ``c_0..c_m`` of Python ints. ``max_mismatches=d`` is the gapped k-mer kernel truncated at d mismatches,
    ``[C(g-h, m-h) if h <= d else 0 for h <= m]``. ``ValueError`` for anything the engine would refuse."""
    from math import comb
    if weights is not None and max_mismatches is not None:
        raise ValueError("give weights= or max_mismatches=, not both")
    if max_mismatches is not None:
        if isinstance(max_mismatches, bool) or not isinstance(max_mismatches, (int, np.integer)):
            raise ValueError("max_mismatches must be an int")
        if not 0 <= int(max_mismatches) <= m:
            raise ValueError("max_mismatches must lie in 0..m = %d, got %d" % (m, int(max_mismatches)))
        weights = [comb(g - h, m - h) if h <= int(max_mismatches) else 0 for h in range(m + 1)]
    if weights is None:
        return None
    if isinstance(weights, (str, bytes)) or not hasattr(weights, "__len__"):
        raise ValueError("weights must be a sequence of m + 1 non-negative ints")
    out = []
    for w in weights:
        if isinstance(w, bool) or not isinstance(w, (int, np.integer)):
            raise ValueError("weights must be non-negative ints, got %r" % (w,))
        if not 0 <= int(w) < 2 ** 64:
            raise ValueError("weights must lie in 0 .. 2^64 - 1, got %r" % (w,))
        out.append(int(w))
    if len(out) != m + 1:
        raise ValueError("weights must hold m + 1 = %d values, got %d" % (m + 1, len(out)))
    if out[0] < 1:
        raise ValueError("weights[0] must be at least 1: it keeps every diagonal positive")
    for j, a in enumerate(solve_mismatch_levels(g, out)):
        if not -2 ** 63 <= a < 2 ** 63:
            raise ValueError("weights: the coefficient of level %d, %d, does not fit 64 bits" % (j, a))
    return out


def flatten(X):
    """Nested int sequences (or a 2-D array) -> (tokens int32, offsets int64)."""
    if isinstance(X, np.ndarray) and X.ndim == 2:
        n, L = X.shape
        return np.ascontiguousarray(X, dtype=np.int32).reshape(-1), np.arange(n + 1, dtype=np.int64) * L
    lens = np.fromiter((len(x) for x in X), dtype=np.int64, count=len(X))
    offsets = np.zeros(len(X) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    tokens = np.empty(int(offsets[-1]), dtype=np.int32)
    for i, x in enumerate(X):
        tokens[offsets[i]:offsets[i + 1]] = x
    return tokens, offsets


class Engine:
    """One engine handle = one device, one HIP stream — or, with ``devices=[...]``, one engine per listed GPU
    of this process behind the same handle (``fsk_create_multi``). Mirrors the C ABI one to one."""

    def __init__(self, g, m, t=-1, approx=False, delta=0.025, max_iters=-1, skip_variance=False, device=0,
                 path=PATH_AUTO, profile=False, lib=None, skip_test_block=False, devices=None, collective=COLL_AUTO,
                 bands=0, deadline_ms=0, tuning=None, revcomp=None, weights=None, max_mismatches=None,
                 wildcards=None, center_weights=None):
        weights = mismatch_weights(g, m, weights, max_mismatches)
        wildcards = wildcard_array(wildcards)
        center_weights = center_weight_array(center_weights)
        if weights is not None and approx:
            raise ValueError("weights= / max_mismatches= with approx=True: a sample of combinations under signed level "
                             "coefficients estimates nothing")
        if weights is not None and devices is not None:
            raise ValueError("weights= / max_mismatches= with devices=[...]: a group of engines does not run the levels")
        self.lib = lib or library()
        if devices is not None:
            devices = [int(d) for d in devices]
            if not devices:
                raise ValueError("devices must list at least one GPU")
            device = devices[0]
        cfg = Config(g=g, m=m, t=t, approx=int(bool(approx)), delta=delta, max_iters=max_iters,
                     skip_variance=int(bool(skip_variance)), device=device, path=path, profile=int(profile),
                     skip_test_block=int(bool(skip_test_block)), collective=int(collective), bands=int(bands),
                     deadline_ms=int(deadline_ms))
        h = C.c_void_p()
        if devices is None:
            rc = self.lib.L.fsk_create(C.byref(cfg), C.byref(h))
        else:
            arr = (C.c_int32 * len(devices))(*devices)
            rc = self.lib.L.fsk_create_multi(C.byref(cfg), arr, len(devices), C.byref(h))
        if rc:
            raise FskError(rc, (self.lib.L.fsk_last_error(None) or b"").decode())
        self.devices = devices
        self.h = h
        self.g, self.m = g, m
        self.device = device
        self._keep = None
        self.revcomp = False
        self.wildcards = []
        self.center_weights = None
        for key, value in (tuning or {}).items():
            self.set_tuning(key, value)
        self.weights = None
        try:
            if revcomp is not None and revcomp is not False:
                self.set_complement(revcomp)
            if len(wildcards):
                self.set_wildcards(wildcards)
            if len(center_weights):
                self.set_center_weights(center_weights)
            if weights is not None:
                self.set_mismatch_weights(weights)
        except Exception:
            self.close()
            raise

    def close(self):
        if getattr(self, "h", None):
            self.lib.L.fsk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc:
            raise FskError(rc, (self.lib.L.fsk_last_error(self.h) or b"").decode())

    # ---- inputs
    @staticmethod
    def _prep(tokens, offsets):
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        return tokens, offsets

    def compute(self, tokens, offsets, n_train, n_test):
        tokens, offsets = self._prep(tokens, offsets)
        self.N, self.n_train, self.n_test = n_train + n_test, n_train, n_test
        self._ck(self.lib.L.fsk_compute(self.h, tokens.ctypes.data, offsets.ctypes.data, n_train, n_test))

    def load_sequences(self, tokens, offsets, n_train, n_test):
        tokens, offsets = self._prep(tokens, offsets)
        self.N, self.n_train, self.n_test = n_train + n_test, n_train, n_test
        self._ck(self.lib.L.fsk_load_sequences(self.h, tokens.ctypes.data, offsets.ctypes.data, n_train, n_test))

    def set_combo_order(self, order):
        order = np.ascontiguousarray(order, dtype=np.int32)
        self._ck(self.lib.L.fsk_set_combo_order(self.h, order.ctypes.data, len(order)))

    def set_seed(self, seed):
        self._ck(self.lib.L.fsk_set_seed(self.h, seed))

    def set_complement(self, mapping):
        """Reverse-complement mode from the next ``load_sequences`` / ``compute`` on: ``mapping`` is the involution
        ``{token_id: token_id}`` (``FastaUtility.complement()``); ``None``, ``False`` or ``{}`` switch it off. A mapping
        that is not one raises ``ValueError``; the engine's own check (``FSK_EINVAL``) is the same."""
        tokens, comps = complement_arrays(mapping)
        self.set_complement_arrays(tokens, comps)

    def set_complement_arrays(self, tokens, complements):
        """``fsk_set_complement`` as it is: two int32 arrays, checked by the engine alone."""
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        complements = np.ascontiguousarray(complements, dtype=np.int32)
        if tokens.shape != complements.shape or tokens.ndim != 1:
            raise ValueError("tokens and complements must be 1-D and of equal length")
        self._ck(self.lib.L.fsk_set_complement(self.h, tokens.ctypes.data, complements.ctypes.data, len(tokens)))
        self.revcomp = len(tokens) > 0

    def set_wildcards(self, wildcards):
        """Wildcard mode from the next ``load_sequences`` / ``compute`` on: a g-window that holds one of the token ids
        ``wildcards`` (``FastaUtility.wildcards()``: the ``n`` of DNA) at any position is not a window. ``None`` or ``[]``
        switch it off. Checked here (``ValueError``) as the engine checks it."""
        self.set_wildcard_array(wildcard_array(wildcards))

    def set_wildcard_array(self, tokens):
        """``fsk_set_wildcards`` as it is: one int32 array, checked by the engine alone."""
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        if tokens.ndim != 1:
            raise ValueError("wildcards must be 1-D")
        self._ck(self.lib.L.fsk_set_wildcards(self.h, tokens.ctypes.data if len(tokens) else None, len(tokens)))
        self.wildcards = sorted(int(t) for t in tokens)

    def set_center_weights(self, center_weights):
        """Centre-weighted mode from the next ``load_sequences`` / ``compute`` on: window p of a sequence of length L counts
        ``w[min(|2p + g - L| // 2, len(w) - 1)]`` times (``center_profile()`` builds such a ``w``). ``None`` or ``[]``
        switch it off. Checked here (``ValueError``) as the engine checks it."""
        self.set_center_weight_array(center_weight_array(center_weights))

    def set_center_weight_array(self, w):
        """``fsk_set_center_weights`` as it is: one uint32 array, checked by the engine alone."""
        w = np.ascontiguousarray(w, dtype=np.uint32)
        if w.ndim != 1:
            raise ValueError("center_weights must be 1-D")
        self._ck(self.lib.L.fsk_set_center_weights(self.h, w.ctypes.data if len(w) else None, len(w)))
        self.center_weights = [int(x) for x in w] if len(w) else None

    def set_mismatch_weights(self, weights):
        """Mismatch-weighted mode from the next ``compute`` on: ``weights`` are ``c_0..c_m`` (``W = sum_h c_h N_h``, N_h the
        pairs of g-windows at exactly h mismatches); ``None`` or ``[]`` switch it off. Checked here (``ValueError``) as the
        engine checks it."""
        if weights is None or len(weights) == 0:
            self._ck(self.lib.L.fsk_set_mismatch_weights(self.h, None, 0))
            self.weights = None
            return
        weights = mismatch_weights(self.g, self.m, weights)
        c = np.array(weights, dtype=np.uint64)
        self._ck(self.lib.L.fsk_set_mismatch_weights(self.h, c.ctypes.data, len(c)))
        self.weights = weights

    def mismatch_info(self):
        """What the last ``compute`` did in mismatch-weighted mode: ``{"n_levels": d + 1, "a": [a_0..a_d], "levels":
        [{"m": j, "k": g - j, "a": a_j, "path": 1 | 2, "ms": host time, "fold_ms": fold time}, ... the levels that ran]}``;
        ``n_levels == 0`` with the mode off."""
        n = C.c_int32(0)
        cap = self.m + 1
        a = np.zeros(cap, dtype=np.int64)
        paths = np.zeros(cap, dtype=np.int32)
        ms = np.zeros(cap, dtype=np.float64)
        fold = np.zeros(cap, dtype=np.float64)
        self._ck(self.lib.L.fsk_get_mismatch_info(self.h, C.byref(n), a.ctypes.data, paths.ctypes.data, cap))
        self._ck(self.lib.L.fsk_get_mismatch_times(self.h, ms.ctypes.data, fold.ctypes.data, cap))
        levels = [{"m": j, "k": self.g - j, "a": int(a[j]), "path": int(paths[j]), "ms": float(ms[j]), "fold_ms": float(fold[j])}
                  for j in range(n.value) if a[j] != 0]
        return {"n_levels": n.value, "a": [int(v) for v in a[:n.value]], "levels": levels}

    # ---- staged path
    def bind_counts(self, device_ptr, n_cells, keepalive=None):
        self._keep = keepalive
        self._ck(self.lib.L.fsk_bind_counts(self.h, C.c_void_p(device_ptr), n_cells))

    def counts_device_ptr(self):
        p = C.c_void_p()
        self._ck(self.lib.L.fsk_counts_device_ptr(self.h, C.byref(p)))
        return p.value

    def reset_counts(self):
        self._ck(self.lib.L.fsk_reset_counts(self.h))

    def reset_counts_rows(self, row_begin, row_end):
        self._ck(self.lib.L.fsk_reset_counts_rows(self.h, row_begin, row_end))

    def accumulate(self, combos):
        combos = np.ascontiguousarray(combos, dtype=np.int32)
        self._ck(self.lib.L.fsk_accumulate(self.h, combos.ctypes.data, len(combos)))

    def accumulate_rows(self, combos, row_begin, row_end):
        combos = np.ascontiguousarray(combos, dtype=np.int32)
        self._ck(self.lib.L.fsk_accumulate_rows(self.h, combos.ctypes.data, len(combos), row_begin, row_end))

    def synchronize(self):
        self._ck(self.lib.L.fsk_synchronize(self.h))

    def stream_wait_engine(self, hip_stream):
        """Work enqueued on ``hip_stream`` (a raw hipStream_t, e.g. ``torch.cuda.current_stream().cuda_stream``)
        from now on waits for what the engine has enqueued so far; the host does not block."""
        self._ck(self.lib.L.fsk_stream_wait_engine(self.h, C.c_void_p(hip_stream)))

    def engine_wait_stream(self, hip_stream):
        """The engine's later work waits for what ``hip_stream`` holds now."""
        self._ck(self.lib.L.fsk_engine_wait_stream(self.h, C.c_void_p(hip_stream)))

    def finalize(self):
        self._ck(self.lib.L.fsk_finalize(self.h))

    # ---- results
    @property
    def pairs(self):
        return self.N * (self.N + 1) // 2

    def get_block(self, i0, i1, j0, j1):
        out = np.empty((i1 - i0, j1 - j0), dtype=np.float64)
        self._ck(self.lib.L.fsk_get_block(self.h, i0, i1, j0, j1, out.ctypes.data))
        return out

    def get_block_torch(self, i0, i1, j0, j1):
        """The normalised block as a float64 torch tensor ON THE GPU (no host round trip)."""
        import torch
        dev = torch.device("cuda", self.device)  # the engine's device, whatever torch's current one is
        out = torch.empty((i1 - i0, j1 - j0), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        self._ck(self.lib.L.fsk_get_block_device(self.h, i0, i1, j0, j1, C.c_void_p(out.data_ptr())))
        return out

    def get_train(self):
        out = np.empty((self.n_train, self.n_train), dtype=np.float64)
        self._ck(self.lib.L.fsk_get_train(self.h, out.ctypes.data))
        return out

    def get_test(self):
        out = np.empty((self.n_test, self.n_train), dtype=np.float64)
        self._ck(self.lib.L.fsk_get_test(self.h, out.ctypes.data))
        return out

    def get_triangle(self):
        out = np.empty(self.pairs, dtype=np.float64)
        self._ck(self.lib.L.fsk_get_triangle(self.h, out.ctypes.data))
        return out

    def get_triangle_torch(self, out=None):
        """The whole normalised triangle as a float64 torch tensor ON THE GPU (pairs doubles, the reference's K)."""
        import torch
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.empty(self.pairs, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        self._ck(self.lib.L.fsk_get_triangle_device(self.h, C.c_void_p(out.data_ptr())))
        return out

    def get_counts(self):
        out = np.empty(self.pairs, dtype=np.uint64)
        self._ck(self.lib.L.fsk_get_counts(self.h, out.ctypes.data))
        return out

    def counts_digest(self, row_begin=0, row_end=None):
        """(sum, xor of cell * (index | 1)) over the integer cells of rows [row_begin, row_end), mod 2^64: an
        order-free digest computed on the device; digests of disjoint row ranges combine by + and ^."""
        out = (C.c_uint64 * 2)()
        self._ck(self.lib.L.fsk_counts_digest(self.h, row_begin, self.N if row_end is None else row_end, out))
        return int(out[0]), int(out[1])

    def multi_info(self):
        info = MultiInfo()
        self._ck(self.lib.L.fsk_get_multi_info(self.h, C.byref(info)))
        return info.as_dict()

    def set_tuning(self, key, value):
        """One knob of the engine (``Library.tuning_keys()`` lists them); never changes a result."""
        self._ck(self.lib.L.fsk_set_tuning(self.h, key.encode(), int(value)))

    def get_tuning(self, key):
        v = C.c_int64(0)
        self._ck(self.lib.L.fsk_get_tuning(self.h, key.encode(), C.byref(v)))
        return int(v.value)

    def set_skip_test_block(self, skip):
        self._ck(self.lib.L.fsk_set_skip_test_block(self.h, int(bool(skip))))

    def get_counts_block(self, i0, i1, j0, j1):
        out = np.empty((i1 - i0, j1 - j0), dtype=np.uint64)
        self._ck(self.lib.L.fsk_get_counts_block(self.h, i0, i1, j0, j1, out.ctypes.data))
        return out

    def get_counts_cells(self, rows, cols):
        """Raw integer cells (rows[q], cols[q]) of the symmetric matrix."""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        cols = np.ascontiguousarray(cols, dtype=np.int64)
        assert rows.shape == cols.shape and rows.ndim == 1
        out = np.empty(len(rows), dtype=np.uint64)
        self._ck(self.lib.L.fsk_get_counts_cells(self.h, rows.ctypes.data, cols.ctypes.data, len(rows), out.ctypes.data))
        return out

    def sequential_sum(self, values):
        """Sum of ``values`` in index order (the reduction of the reference's get_variance), on the device."""
        values = np.ascontiguousarray(values, dtype=np.float64)
        out = C.c_double(0.0)
        self._ck(self.lib.L.fsk_sequential_sum(self.h, values.ctypes.data, len(values), C.byref(out)))
        return out.value

    # ---- variance mode over several engines: the Welford chains are the units
    def run_chains(self, first, step):
        """Chains ``first, first + step, ...`` of the ``t`` Welford chains (after ``load_sequences``)."""
        self._ck(self.lib.L.fsk_run_chains(self.h, first, step))

    def get_kernel_sum_device(self, device_ptr):
        """The fp64 sum of the chains' K_hat into ``pairs`` doubles at ``device_ptr`` (device memory)."""
        self._ck(self.lib.L.fsk_get_kernel_sum_device(self.h, C.c_void_p(device_ptr)))

    def set_kernel_sum_device(self, device_ptr):
        self._ck(self.lib.L.fsk_set_kernel_sum_device(self.h, C.c_void_p(device_ptr)))

    def get_stdevs(self):
        n = C.c_int32(0)
        self._ck(self.lib.L.fsk_get_stdevs(self.h, None, 0, C.byref(n)))
        out = np.empty(max(n.value, 1), dtype=np.float64)
        self._ck(self.lib.L.fsk_get_stdevs(self.h, out.ctypes.data, n.value, C.byref(n)))
        return out[:n.value]

    def save_kernel(self, path):
        self._ck(self.lib.L.fsk_save_kernel(self.h, path.encode()))

    # ---- the SVM stage on the resident triangle
    def svm_train(self, labels, C=1.0, eps=1e-3, max_iter=-1):
        """``fsk_svm_train``: a C-SVC on the train x train part of the finalized result, ``labels`` in {-1, +1}. Returns the
        info of the solve (``svm_model()[2]``)."""
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if labels.ndim != 1:
            raise ValueError("labels must be 1-D")
        self._ck(self.lib.L.fsk_svm_train(self.h, labels.ctypes.data if len(labels) else None, len(labels), float(C), float(eps),
                                          int(max_iter)))
        return self.svm_model()[2]

    def svm_model(self):
        """(alpha[n_train], rho, info dict) of the last ``svm_train``."""
        alpha = np.empty(self.n_train, dtype=np.float64)
        rho = C.c_double(0.0)
        info = SvmInfo()
        self._ck(self.lib.L.fsk_svm_get_model(self.h, alpha.ctypes.data, C.byref(rho), C.byref(info)))
        return alpha, rho.value, info.as_dict()

    def svm_decision(self, r0, r1):
        """Decision values of rows [r0, r1) of the sequences (train rows first)."""
        out = np.empty(max(r1 - r0, 0), dtype=np.float64)
        self._ck(self.lib.L.fsk_svm_decision(self.h, r0, r1, out.ctypes.data))
        return out

    def svm_cv(self, labels, fold, Cs, eps=1e-3, max_iter=-1, n_folds=None):
        """``fsk_svm_cv``: the C-SVC cross-validated over the folds ``fold[t]`` (0..F-1; F = ``n_folds``, the largest id + 1 when None) and the values ``Cs``,
        every (C, fold) problem solved side by side. Returns ``decision`` [n_C, n_train] (out-of-fold), ``auc`` and
        ``accuracy`` [n_C], ``problems`` (problem ``c * F + f``: C index c, fold f held out), ``form``, ``launches``, ``ms``."""
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        fold = np.ascontiguousarray(fold, dtype=np.int32)
        Cs = np.ascontiguousarray(Cs, dtype=np.float64)
        if labels.ndim != 1 or fold.ndim != 1 or Cs.ndim != 1:
            raise ValueError("labels, fold and Cs must be 1-D")
        if len(fold) != len(labels):
            raise ValueError("%d fold ids for %d labels" % (len(fold), len(labels)))
        if n_folds is None:
            n_folds = int(fold.max()) + 1 if len(fold) else 0
        ptr = lambda a: a.ctypes.data if len(a) else None
        self._ck(self.lib.L.fsk_svm_cv(self.h, ptr(labels), len(labels), ptr(fold), n_folds, ptr(Cs), len(Cs), float(eps), int(max_iter)))
        n, P = len(labels), len(Cs) * n_folds
        oof = np.empty((len(Cs), n), dtype=np.float64)
        scores, problems, info = (SvmCvScore * len(Cs))(), (SvmCvProblem * P)(), SvmCvInfo()
        self._ck(self.lib.L.fsk_svm_cv_get(self.h, oof.ctypes.data, C.addressof(scores), C.addressof(problems), C.byref(info)))
        return {"decision": oof, "auc": np.array([s.auc for s in scores]), "accuracy": np.array([s.accuracy for s in scores]),
                "problems": [q.as_dict() for q in problems], "form": _FORMS.get(info.form, "none"), "launches": info.launches,
                "ms": info.ms}

    # ---- epsilon-SVR on the resident triangle (the model slot is the C-SVC's: svm_decision serves either)
    def svr_train(self, targets, C=1.0, epsilon=0.1, eps=1e-3, max_iter=-1):
        """``fsk_svr_train``: an epsilon-SVR on the train x train part of the finalized result, ``targets`` real-valued.
        Returns the info of the solve (``svr_model()[3]``)."""
        targets = np.ascontiguousarray(targets, dtype=np.float64)
        if targets.ndim != 1:
            raise ValueError("targets must be 1-D")
        self._ck(self.lib.L.fsk_svr_train(self.h, targets.ctypes.data if len(targets) else None, len(targets), float(C), float(epsilon),
                                          float(eps), int(max_iter)))
        return self.svr_model()[3]

    def svr_model(self):
        """(alpha2[2 n_train]: alpha then alpha*, coef[n_train] = alpha - alpha*, rho, info dict) of the last ``svr_train``."""
        alpha2 = np.empty(2 * self.n_train, dtype=np.float64)
        coef = np.empty(self.n_train, dtype=np.float64)
        rho = C.c_double(0.0)
        info = SvmInfo()
        self._ck(self.lib.L.fsk_svr_get_model(self.h, alpha2.ctypes.data, coef.ctypes.data, C.byref(rho), C.byref(info)))
        return alpha2, coef, rho.value, info.as_dict()

    def svr_cv(self, targets, fold, Cs, epsilons, eps=1e-3, max_iter=-1, n_folds=None):
        """``fsk_svr_cv``: the epsilon-SVR cross-validated over the folds ``fold[t]`` (0..F-1; F = ``n_folds``, the largest id
        + 1 when None) and the grid ``Cs`` x ``epsilons``, every problem solved side by side. Returns ``oof``
        [n_C, n_eps, n_train] (out-of-fold predictions), ``mse``, ``mae``, ``r2``, ``r`` [n_C, n_eps], ``problems`` (problem
        ``(c * n_eps + q) * F + f``: with ``epsilon``), ``form``, ``launches``, ``ms``."""
        targets = np.ascontiguousarray(targets, dtype=np.float64)
        fold = np.ascontiguousarray(fold, dtype=np.int32)
        Cs = np.ascontiguousarray(Cs, dtype=np.float64)
        epsilons = np.ascontiguousarray(epsilons, dtype=np.float64)
        if targets.ndim != 1 or fold.ndim != 1 or Cs.ndim != 1 or epsilons.ndim != 1:
            raise ValueError("targets, fold, Cs and epsilons must be 1-D")
        if len(fold) != len(targets):
            raise ValueError("%d fold ids for %d targets" % (len(fold), len(targets)))
        if n_folds is None:
            n_folds = int(fold.max()) + 1 if len(fold) else 0
        ptr = lambda a: a.ctypes.data if len(a) else None
        self._ck(self.lib.L.fsk_svr_cv(self.h, ptr(targets), len(targets), ptr(fold), n_folds, ptr(Cs), len(Cs), ptr(epsilons), len(epsilons),
                                       float(eps), int(max_iter)))
        n, nC, nE = len(targets), len(Cs), len(epsilons)
        oof = np.empty((nC, nE, n), dtype=np.float64)
        scores, problems, info = (SvrCvScore * (nC * nE))(), (SvmCvProblem * (nC * nE * n_folds))(), SvmCvInfo()
        self._ck(self.lib.L.fsk_svr_cv_get(self.h, oof.ctypes.data, C.addressof(scores), C.addressof(problems), C.byref(info)))
        out = {k: np.array([getattr(s, k) for s in scores]).reshape(nC, nE) for k in ("mse", "mae", "r2", "r")}
        out.update({"oof": oof, "problems": [dict(q.as_dict(), epsilon=q.reserved[0]) for q in problems],
                    "form": _FORMS.get(info.form, "none"), "launches": info.launches, "ms": info.ms})
        return out

    # ---- the rows kernel: L(r, c) = <K(r, train), K(c, train)> of the finalized result, K2 its cosine normalisation
    def rows_build(self):
        """``fsk_rows_build``: build the rows kernel of the finalized result (nothing when it is there). Returns ``rows_info()``."""
        self._ck(self.lib.L.fsk_rows_build(self.h))
        return self.rows_info()

    def rows_block(self, i0, i1, j0, j1, raw=False):
        """Cells [i0, i1) x [j0, j1) of the rows kernel, either order of (r, c): L when ``raw``, else K2. Does not build."""
        out = np.empty((max(i1 - i0, 0), max(j1 - j0, 0)), dtype=np.float64)
        self._ck(self.lib.L.fsk_rows_get_block(self.h, i0, i1, j0, j1, int(bool(raw)), out.ctypes.data))
        return out

    def rows_info(self):
        info = RowsInfo()
        self._ck(self.lib.L.fsk_rows_get_info(self.h, C.byref(info)))
        return info.as_dict()

    def svm_set_kernel(self, kind):
        """What ``svm_train`` / ``svm_cv`` solve on: ``SVM_KERNEL_RESULT`` / "fastsk" (the default) or ``SVM_KERNEL_ROWS`` /
        "linear". A change drops the model and the cross-validation result."""
        if isinstance(kind, str):
            if kind not in _SVM_KERNELS:
                raise ValueError("kernel kind %r: one of %s" % (kind, sorted(_SVM_KERNELS)))
            kind = _SVM_KERNELS[kind]
        self._ck(self.lib.L.fsk_svm_set_kernel(self.h, int(kind)))

    def svm_get_kernel(self):
        v = C.c_int32(0)
        self._ck(self.lib.L.fsk_svm_get_kernel(self.h, C.byref(v)))
        return int(v.value)

    def svm_set_class_weights(self, w_pos, w_neg):
        """``fsk_svm_set_class_weights``: from now on ``svm_train`` and ``svm_cv`` solve with the boxes ``C w_pos`` for the rows
        of label +1 and ``C w_neg`` for label -1 (``class_weights(labels, spec)`` makes the pair). A change drops the model,
        the cross-validation result and the calibration; the weights stay with the handle."""
        self._ck(self.lib.L.fsk_svm_set_class_weights(self.h, float(w_pos), float(w_neg)))

    def svm_get_class_weights(self):
        wp, wn = C.c_double(0.0), C.c_double(0.0)
        self._ck(self.lib.L.fsk_svm_get_class_weights(self.h, C.byref(wp), C.byref(wn)))
        return wp.value, wn.value

    def svm_calibrate(self, fold, n_folds=None):
        """``fsk_svm_calibrate``: Platt's sigmoid for the model of ``svm_train``, fitted on the out-of-fold decision values of
        the folds ``fold[t]`` (0..F-1; F = ``n_folds``, the largest id + 1 when None) solved side by side with the model's C,
        eps, max_iter, class weights and kernel kind. Returns ``svm_calibration()[1]``."""
        fold = np.ascontiguousarray(fold, dtype=np.int32)
        if fold.ndim != 1:
            raise ValueError("fold must be 1-D")
        if n_folds is None:
            n_folds = int(fold.max()) + 1 if len(fold) else 0
        if len(fold) != self.n_train:
            raise ValueError("%d fold ids for %d training sequences" % (len(fold), self.n_train))
        self._ck(self.lib.L.fsk_svm_calibrate(self.h, fold.ctypes.data if len(fold) else None, int(n_folds)))
        return self.svm_calibration()[1]

    def svm_calibration(self):
        """(the out-of-fold decision values [n_train], the fit: ``A``, ``B``, ``iterations``, ``status``, ``n_folds``,
        ``form``, ``launches``, ``ms``) of the last ``svm_calibrate``."""
        oof = np.empty(self.n_train, dtype=np.float64)
        info = SvmPlattInfo()
        self._ck(self.lib.L.fsk_svm_get_calibration(self.h, oof.ctypes.data, C.byref(info)))
        return oof, info.as_dict()

    def svm_proba(self, r0, r1):
        """P(y = +1) of rows [r0, r1) of the sequences (train rows first): the calibration's sigmoid of ``svm_decision``."""
        out = np.empty(max(r1 - r0, 0), dtype=np.float64)
        self._ck(self.lib.L.fsk_svm_proba(self.h, r0, r1, out.ctypes.data))
        return out

    # ---- multi-class C-SVC, one-vs-one: the pairs of classes as one batch on the resident triangle
    def _class_weight_array(self, labels, class_weight):
        """``class_weight`` for the C calls: None, or one weight a class in ascending class order (an array, or "balanced" / a
        dict keyed by label through ``multiclass_weights``)."""
        if class_weight is None:
            return None
        if hasattr(class_weight, "items") or isinstance(class_weight, str):
            return multiclass_weights(labels, class_weight)
        w = np.ascontiguousarray(class_weight, dtype=np.float64)
        if w.ndim != 1 or len(w) != len(np.unique(labels)):
            raise ValueError("class_weight: one weight a class, in ascending class order")
        return w

    def svm_train_multiclass(self, labels, C=1.0, eps=1e-3, max_iter=-1, class_weight=None):
        """``fsk_svm_train_multiclass``: a one-vs-one C-SVC on the train x train part of the finalized result, ``labels`` any
        int32 values (2 to 64 classes). ``class_weight``: None, one weight a class in ascending class order, or what
        ``multiclass_weights`` takes ("balanced", a dict keyed by label). Returns the info of ``svm_multiclass_model()``."""
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if labels.ndim != 1:
            raise ValueError("labels must be 1-D")
        w = self._class_weight_array(labels, class_weight)
        self._ck(self.lib.L.fsk_svm_train_multiclass(self.h, labels.ctypes.data if len(labels) else None, len(labels), float(C),
                                                     None if w is None else w.ctypes.data, float(eps), int(max_iter)))
        return self.svm_multiclass_model()["info"]

    def svm_multiclass_model(self):
        """The model of the last ``svm_train_multiclass``: ``classes`` [k] ascending, ``pairs`` (pair p over classes (a, b),
        a < b, lexicographic: ``class_a``, ``class_b``, ``n_rows``, ``iterations``, ``gap``, ``objective``, ``rho``, ``n_sv``,
        ``n_bsv``, ``converged``), ``alpha`` (a list: pair p's alpha at its own length, over its rows ascending) and ``info``
        (``k``, ``n_pairs``, ``form``, ``launches``, ``ms``, ``n_sv``: rows that are a support vector of any pair)."""
        info = SvmMulticlassInfo()
        self._ck(self.lib.L.fsk_svm_multiclass_get_model(self.h, None, None, None, C.byref(info)))
        classes = np.empty(info.k, dtype=np.int32)
        pairs = (SvmMulticlassPair * info.n_pairs)()
        alpha = np.empty(info.n_alpha, dtype=np.float64)
        self._ck(self.lib.L.fsk_svm_multiclass_get_model(self.h, classes.ctypes.data, C.addressof(pairs), alpha.ctypes.data, C.byref(info)))
        cuts = np.cumsum([q.n_rows for q in pairs])[:-1]
        return {"classes": classes, "pairs": [q.as_dict() for q in pairs], "alpha": np.split(alpha, cuts), "info": info.as_dict()}

    def svm_multiclass_decision(self, r0, r1, decision=True, predict=True):
        """``fsk_svm_multiclass_decision``: (the pairs' decision values [r1 - r0, P], the winning labels [r1 - r0]) of rows
        [r0, r1) of the sequences (train rows first); None for the one not asked for."""
        info = SvmMulticlassInfo()
        self._ck(self.lib.L.fsk_svm_multiclass_get_model(self.h, None, None, None, C.byref(info)))
        rows = max(r1 - r0, 0)
        dec = np.empty((rows, info.n_pairs), dtype=np.float64) if decision else None
        pred = np.empty(rows, dtype=np.int32) if predict else None
        self._ck(self.lib.L.fsk_svm_multiclass_decision(self.h, r0, r1, None if dec is None else dec.ctypes.data,
                                                        None if pred is None else pred.ctypes.data))
        return dec, pred

    def svm_multiclass_cv(self, labels, fold, Cs, eps=1e-3, max_iter=-1, n_folds=None, class_weight=None):
        """``fsk_svm_multiclass_cv``: the one-vs-one C-SVC cross-validated over the folds ``fold[t]`` and the values ``Cs``, every
        (C, fold, pair) problem solved side by side. Returns ``pred`` [n_C, n_train] (out-of-fold labels), ``accuracy`` [n_C]
        (there is no AUC for more than two classes), ``problems`` (problem ``(c * F + f) * P + p`` with ``class_a``,
        ``class_b``), ``k``, ``form``, ``launches``, ``ms``."""
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        fold = np.ascontiguousarray(fold, dtype=np.int32)
        Cs = np.ascontiguousarray(Cs, dtype=np.float64)
        if labels.ndim != 1 or fold.ndim != 1 or Cs.ndim != 1:
            raise ValueError("labels, fold and Cs must be 1-D")
        if len(fold) != len(labels):
            raise ValueError("%d fold ids for %d labels" % (len(fold), len(labels)))
        if n_folds is None:
            n_folds = int(fold.max()) + 1 if len(fold) else 0
        w = self._class_weight_array(labels, class_weight)
        ptr = lambda a: a.ctypes.data if len(a) else None
        self._ck(self.lib.L.fsk_svm_multiclass_cv(self.h, ptr(labels), len(labels), ptr(fold), n_folds, ptr(Cs), len(Cs),
                                                  None if w is None else w.ctypes.data, float(eps), int(max_iter)))
        info = SvmCvInfo()
        self._ck(self.lib.L.fsk_svm_multiclass_cv_get(self.h, None, None, None, C.byref(info)))
        k = info.reserved0
        n, total = len(labels), len(Cs) * n_folds * (k * (k - 1) // 2)
        pred = np.empty((len(Cs), n), dtype=np.int32)
        scores, problems = (SvmCvScore * len(Cs))(), (SvmCvProblem * total)()
        self._ck(self.lib.L.fsk_svm_multiclass_cv_get(self.h, pred.ctypes.data, C.addressof(scores), C.addressof(problems), C.byref(info)))
        return {"pred": pred, "accuracy": np.array([s.accuracy for s in scores]),
                "problems": [dict(q.as_dict(), class_a=int(q.reserved[0]), class_b=int(q.reserved[1])) for q in problems], "k": k,
                "form": _FORMS.get(info.form, "none"), "launches": info.launches, "ms": info.ms}

    def svm_multiclass_calibrate(self, fold, n_folds=None):
        """``fsk_svm_multiclass_calibrate``: a Platt sigmoid for every pair of the model of ``svm_train_multiclass``, fitted on
        the out-of-fold pair decisions of the folds ``fold[t]`` (0..F-1; F = ``n_folds``, the largest id + 1 when None), all
        F * P problems solved side by side with the model's C, class weights, eps, max_iter and kernel kind. Returns
        ``svm_multiclass_calibration()[1]``."""
        fold = np.ascontiguousarray(fold, dtype=np.int32)
        if fold.ndim != 1:
            raise ValueError("fold must be 1-D")
        if n_folds is None:
            n_folds = int(fold.max()) + 1 if len(fold) else 0
        if len(fold) != self.n_train:
            raise ValueError("%d fold ids for %d training sequences" % (len(fold), self.n_train))
        self._ck(self.lib.L.fsk_svm_multiclass_calibrate(self.h, fold.ctypes.data if len(fold) else None, int(n_folds)))
        return self.svm_multiclass_calibration()[1]

    def svm_multiclass_calibration(self):
        """(the out-of-fold pair decisions [n_train, P] — None where ``svm_multiclass_set_calibration`` installed the sigmoids —
        and the P fits: ``A``, ``B``, ``iterations``, ``status``, ``n_folds``, ``form``, ``launches``, ``ms``)."""
        info = SvmMulticlassInfo()
        self._ck(self.lib.L.fsk_svm_multiclass_get_model(self.h, None, None, None, C.byref(info)))
        fits = (SvmPlattInfo * info.n_pairs)()
        self._ck(self.lib.L.fsk_svm_multiclass_get_calibration(self.h, None, C.addressof(fits)))
        oof = None
        if fits[0].n_folds:
            oof = np.empty((self.n_train, info.n_pairs), dtype=np.float64)
            self._ck(self.lib.L.fsk_svm_multiclass_get_calibration(self.h, oof.ctypes.data, None))
        return oof, [f.as_dict() for f in fits]

    def svm_multiclass_set_calibration(self, A, B):
        """``fsk_svm_multiclass_set_calibration``: install the sigmoids ``A[p]``, ``B[p]`` of the P pairs without a solve."""
        info = SvmMulticlassInfo()
        self._ck(self.lib.L.fsk_svm_multiclass_get_model(self.h, None, None, None, C.byref(info)))
        A = np.ascontiguousarray(A, dtype=np.float64)
        B = np.ascontiguousarray(B, dtype=np.float64)
        if A.shape != (info.n_pairs,) or B.shape != (info.n_pairs,):
            raise ValueError("A and B: one value a pair, %d pairs" % info.n_pairs)
        self._ck(self.lib.L.fsk_svm_multiclass_set_calibration(self.h, A.ctypes.data, B.ctypes.data))

    def svm_multiclass_proba(self, r0, r1, proba=True, predict=True, iterations=True):
        """``fsk_svm_multiclass_proba``: (the class probabilities [r1 - r0, k] in the order of ``classes``, the label of the
        largest [r1 - r0], the coupling's iterations [r1 - r0]) of rows [r0, r1); None for what is not asked for."""
        info = SvmMulticlassInfo()
        self._ck(self.lib.L.fsk_svm_multiclass_get_model(self.h, None, None, None, C.byref(info)))
        rows = max(r1 - r0, 0)
        prob = np.empty((rows, info.k), dtype=np.float64) if proba else None
        pred = np.empty(rows, dtype=np.int32) if predict else None
        iters = np.empty(rows, dtype=np.int32) if iterations else None
        ptr = lambda a: None if a is None else a.ctypes.data
        self._ck(self.lib.L.fsk_svm_multiclass_proba(self.h, r0, r1, ptr(prob), ptr(pred), ptr(iters)))
        return prob, pred, iters

    def svm_cv_alpha(self, p):
        """alpha[n_train] of problem ``p`` of the last ``svm_cv``, zero at its held-out rows."""
        out = np.empty(self.n_train, dtype=np.float64)
        self._ck(self.lib.L.fsk_svm_cv_get_alpha(self.h, int(p), out.ctypes.data))
        return out

    def stats(self):
        s = Stats()
        self._ck(self.lib.L.fsk_get_stats(self.h, C.byref(s)))
        d = s.as_dict()
        d["revcomp"] = self.revcomp  # (as set: in force from the next load on)
        d["wildcards"] = list(self.wildcards)
        d["center_weights"] = None if self.center_weights is None else list(self.center_weights)
        d["weights"] = None if self.weights is None else list(self.weights)  # (mismatch-weighted mode, as set)
        return d
