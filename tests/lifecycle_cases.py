"""Inputs of the engine-lifecycle scenarios (create -> load -> run -> destroy), shared by tests/test_emu_lifecycle.py — which
counts what the emulated HIP runtime has handed out and not taken back — and tests/test_gpu_lifecycle.py. Nothing here touches
an engine. Every scenario runs on a small golden of tests/golden or on a case of another case module, so each has a value to
be compared with: a scenario cannot pass by doing nothing."""
import numpy as np

from conftest import load_golden

DENSE = "f3_lowcomplexity_g5m2"        # DNA, g = 5, m = 2: 10 combinations, dense dataflow
SPARSE = "f8_sigma300_g5m2"            # 300 symbols, g = 5, m = 2, N = 80: sparse dataflow whatever the tuning
VARIANCE = "f4_ep300_variance_T1"
SKIPVAR = "f6_prot219_skipvar16"
GROUP = "f4_ep300_exact"               # N = 100, 210 combinations
TWO_LOADS = ((1, "f3_ragged_sigma7_g6m3", 5), (2, SPARSE, 37))   # (dataflow, golden, sequences of the smaller load)

# two-level blocks in several passes on 3240 cells: two bands a pass, sub-bands of 16 cells — and bands of 1024 cells at most,
# without which two bands take all of a triangle this small and the pass is one
BLOCKS_TUNING = {"sparse_form": 2, "blocks_max_bands": 2, "blocks_sub_shift": 4, "blocks_band_shift_max": 10}
INITIAL_STATS = {"sparse_passes": 0, "sparse_form": -1, "sparse_desc": 0, "share_positions": 0, "share_groups": 0}
PER_LOAD_STATS = tuple(INITIAL_STATS)


def n_features(d):
    """g-windows of all sequences of a golden: the sort records of one combination."""
    lens = np.diff(d["offsets"])
    return int(np.maximum(lens - d["g"] + 1, 0).sum())


def lanes_tuning(d):
    """Two combinations a batch, the batches of an exact accumulate in two lanes."""
    return {"sparse_exact_lanes": 2, "sparse_batch_records": 2 * n_features(d)}


def prefix(d, n):
    """The first n sequences of a golden, all of them training rows, and their cells: rows 0 .. n - 1 of the packed lower
    triangle are its first n (n + 1) / 2 cells."""
    off = d["offsets"][:n + 1]
    return d["tokens"][:off[-1]], off, d["counts"][:n * (n + 1) // 2]


def golden(name):
    return load_golden(name)
