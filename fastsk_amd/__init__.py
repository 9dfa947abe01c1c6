"""fastsk_amd — MI355X-native gapped-k-mer string-kernel engine (drop-in for QData/FastSK's
``FastSK(g, m, ...).compute_kernel(Xtrain, Xtest)`` path)."""
from .utils import FastaUtility, Vocabulary  # noqa: F401

__all__ = ["FastSK", "FastaUtility", "Vocabulary", "mismatch_levels", "center_profile", "stratified_folds", "kfold", "class_weights",
           "multiclass_weights"]


def __getattr__(name):
    # The pybind11 class needs the HIP library; import it lazily so that the pure-Python helpers
    # (FASTA reader, ctypes view) stay importable on a box where the engine is not built yet.
    if name == "FastSK":
        from ._native import share_hip_runtime_with_torch
        share_hip_runtime_with_torch()  # before the extension pulls in libamdhip64
        from ._fastsk import FastSK
        return FastSK
    if name == "mismatch_levels":  # (host only, but it lives in the HIP library)
        from ._native import mismatch_levels
        return mismatch_levels
    if name == "center_profile":  # (host only, pure Python)
        from ._native import center_profile
        return center_profile
    if name == "stratified_folds":  # (host only, pure Python)
        from ._native import stratified_folds
        return stratified_folds
    if name == "kfold":  # (host only, pure Python)
        from ._native import kfold
        return kfold
    if name == "class_weights":  # (host only, pure Python)
        from ._native import class_weights
        return class_weights
    if name == "multiclass_weights":  # (host only, pure Python)
        from ._native import multiclass_weights
        return multiclass_weights
    raise AttributeError(name)
