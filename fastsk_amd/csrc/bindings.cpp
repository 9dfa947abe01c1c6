// bindings.cpp — pybind11 module `fastsk_amd._fastsk`: the reference's Python surface
// (QData/FastSK src/fastsk/_fastsk/bindings.cpp:12-51) on top of the C ABI in
// include/fastsk_amd.h. Same class name, constructor keywords and defaults, method names and
// return types; host C++ only — all computation happens behind fsk_* in libfastsk_amd.so.
//
// Deviations, all documented in INTEGRATION.md:
//   - errors raise ValueError / RuntimeError instead of printf + exit(1) (fastsk.cpp:53-58);
//   - fit() / score() (LIBSVM, fastsk.cpp:239-530) are outside this path and raise
//     NotImplementedError (they are unusable from Python in the reference as well); the SVM stage is additive instead:
//     fit_svm(labels, C, eps, max_iter), get_dual_coef_np(), get_intercept(), decision_function_np / _dlpack(which) train
//     and score a C-SVC on the triangle the compute call left on the device (fsk_svm_train / fsk_svm_decision), and
//     cross_validate_svm(labels, Cs, folds, ...) cross-validates it over folds and values of C in one batch (fsk_svm_cv);
//     class_weight= on both gives LIBSVM's weighted C-SVC (fsk_svm_set_class_weights), fit_svm(probability=True) and
//     predict_proba_np(which) Platt's probabilities (fsk_svm_calibrate / fsk_svm_proba);
//     fit_svr(targets, C, epsilon, ...), predict_np / predict_dlpack(which) and cross_validate_svr(targets, Cs, epsilons, folds, ...)
//     the epsilon-SVR on real-valued targets (fsk_svr_train / fsk_svr_cv), in the one model slot;
//     fit_svm_multiclass(labels, C, ...), predict_class_np(which) and cross_validate_svm_multiclass(labels, Cs, folds, ...) the
//     one-vs-one multi-class C-SVC on integer labels (fsk_svm_train_multiclass / fsk_svm_multiclass_cv), in the same slot;
//     fit_svm_multiclass(probability=True), predict_proba_np / predict_proba_dlpack(which) and predict_class_np(rule="proba") its
//     class probabilities by pairwise coupling (fsk_svm_multiclass_calibrate / fsk_svm_multiclass_proba);
//     all of them take a trailing kernel_type = "fastsk" | "linear": "linear" is the reference's default, the SVM on the ROWS of
//     the kernel, through the rows kernel (fsk_rows_build; get_rows_kernel_block_np, rows_kernel_info);
//   - additive keyword arguments (device, devices, collective, deadline_ms, path, seed, skip_test_block, revcomp, weights, max_mismatches, wildcards, center_weights), numpy and
//     DLPack getters. devices=[0,1,...]: one engine per listed GPU behind the same object (fsk_create_multi) —
//     the reference parallelises the same call over t host threads (fastsk_kernel.cpp:54-93).
//   - skip_test_block (default False: compute_kernel computes the whole N x N triangle, as fastsk.cpp:30-118 does).
//     The test x test block, which no getter of the reference exposes (fastsk.cpp:190-217), can be left out:
//     skip_test_block=True never computes it (its cells read as zero); skip_test_block="lazy" (or None) leaves it
//     out of compute_kernel and the first request that needs it (get_block over test x test cells, get_counts_np,
//     counts_digest over test rows, get_triangle_dlpack, save_kernel) runs the whole compute once more with
//     nothing left out — about twice the time of compute_kernel in total; the object keeps the tokens until then.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

//   - revcomp (default None: off): the complement mapping {token_id: token_id} of reverse-complement mode
//     (fsk_set_complement; FastaUtility.complement() returns it for DNA) — a k-mer is counted together with its reverse
//     complement, as gkm-SVM / LS-GKM do; the reference has no such mode.
//   - weights / max_mismatches (default None: off): the mismatch-weighted kernels of fsk_set_mismatch_weights —
//     weights = c_0..c_m, W = sum_h c_h N_h over the pairs of g-windows at exactly h mismatches; max_mismatches = d is
//     shorthand for the gapped k-mer kernel truncated at d mismatches, c_h = C(g-h, m-h) for h <= d and 0 beyond (LS-GKM's
//     "-l g -k g-m -d d"). Checked before any device call (ValueError); not with approx=True or devices=[...].
//   - wildcards (default None: off): token ids that stand for "unknown" (fsk_set_wildcards; FastaUtility.wildcards() returns
//     the id of DNA's n) — a g-window that holds one at any position is not a window, as in every k-mer tool; the reference
//     has no such mode and matches n with n. Checked before any device call (ValueError).
//   - center_weights (default None: off): a profile w of at most 4096 integers in 0..255, w[0] >= 1 (fsk_set_center_weights;
//     fastsk_amd.center_profile() builds one) — window p of a sequence of length L counts w[min(|2p + g - L| / 2, len(w) - 1)]
//     times, the centre-weighted gapped k-mer kernel (LS-GKM's "-t 4"); the reference weighs every window 1. Checked before
//     any device call (ValueError). Keyword-only, in an overload of its own: the signature that ends in wildcards stays as it
//     was, by position too.
#include "../../include/fastsk_amd.h"

namespace py = pybind11;

namespace {

struct Flat {
    std::vector<int32_t> tokens;
    std::vector<int64_t> offsets{0};
    // The rows of X — what FastaUtility.read_data returns (a list of lists of ints), or any sequence of sequences, of int32
    // arrays, or a 2-D integer array — straight into the packed token buffer: the reference's signature copies a
    // std::vector<std::vector<int>> by value (fastsk.cpp:30), i.e. every token twice through pybind's generic casters before
    // the engine sees it; here a list row is one PyLong_AsLong per token and an int32 array row one memcpy.
    size_t add(const py::handle& X) {
        if (py::isinstance<py::array>(X)) {
            auto a = py::array_t<int32_t, py::array::c_style | py::array::forcecast>::ensure(X);
            if (a && a.ndim() == 2) {
                const py::ssize_t n = a.shape(0), L = a.shape(1);
                tokens.insert(tokens.end(), a.data(), a.data() + n * L);
                for (py::ssize_t i = 0; i < n; ++i) offsets.push_back(offsets.back() + L);
                return (size_t)n;
            }
        }
        PyObject* seq = PySequence_Fast(X.ptr(), "expected a sequence of token sequences");
        if (!seq) throw py::error_already_set();
        py::object hold = py::reinterpret_steal<py::object>(seq);
        const Py_ssize_t n = PySequence_Fast_GET_SIZE(seq);
        PyObject** rows = PySequence_Fast_ITEMS(seq);
        {   // one reservation for every row whose length is cheap to ask for
            size_t total = tokens.size();
            for (Py_ssize_t i = 0; i < n; ++i) {
                const Py_ssize_t len = PyObject_Length(rows[i]);
                if (len < 0) { PyErr_Clear(); continue; }
                total += (size_t)len;
            }
            tokens.reserve(total);
        }
        for (Py_ssize_t i = 0; i < n; ++i) {
            PyObject* r = rows[i];
            if (PyList_CheckExact(r) || PyTuple_CheckExact(r)) {
                const Py_ssize_t len = PySequence_Fast_GET_SIZE(r);
                PyObject** it = PySequence_Fast_ITEMS(r);
                const size_t at = tokens.size();
                tokens.resize(at + (size_t)len);
                int32_t* dst = tokens.data() + at;
                for (Py_ssize_t q = 0; q < len; ++q) {
                    const long v = PyLong_AsLong(it[q]);
                    if (v == -1 && PyErr_Occurred()) throw py::error_already_set();
                    if (v < INT32_MIN || v > INT32_MAX) throw py::value_error("token ids must fit 32 bits");
                    dst[q] = (int32_t)v;
                }
            } else {  // an array (or any other sequence) row
                auto a = py::array_t<int32_t, py::array::c_style | py::array::forcecast>::ensure(py::handle(r));
                if (!a || a.ndim() != 1) { PyErr_Clear(); throw py::value_error("every sequence must be a list, a tuple or a 1-D array of token ids"); }
                tokens.insert(tokens.end(), a.data(), a.data() + a.shape(0));
            }
            offsets.push_back((int64_t)tokens.size());
        }
        return (size_t)n;
    }
};

// ---- DLPack (the ABI of dlpack.h v0.8, restated: nothing else of it is needed here) --------------------
struct DLDevice { int32_t device_type; int32_t device_id; };
struct DLDataType { uint8_t code; uint8_t bits; uint16_t lanes; };
struct DLTensor {
    void* data; DLDevice device; int32_t ndim; DLDataType dtype; int64_t* shape; int64_t* strides; uint64_t byte_offset;
};
struct DLManagedTensor { DLTensor dl_tensor; void* manager_ctx; void (*deleter)(DLManagedTensor*); };
constexpr int32_t kDLROCM = 10;
constexpr uint8_t kDLFloat = 2;
struct BlockOwner { int64_t shape[2]; };   // manager_ctx of a block handed out through DLPack

int parse_collective(const std::string& c) {
    if (c == "auto") return FSK_COLL_AUTO;
    if (c == "rccl") return FSK_COLL_RCCL;
    if (c == "p2p") return FSK_COLL_P2P;
    throw std::invalid_argument("collective must be 'auto', 'rccl' or 'p2p'");
}

int parse_path(const std::string& p) {
    if (p == "auto") return FSK_PATH_AUTO;
    if (p == "dense") return FSK_PATH_DENSE;
    if (p == "sparse") return FSK_PATH_SPARSE;
    throw std::invalid_argument("path must be 'auto', 'dense' or 'sparse'");
}

class FastSK {
    fsk_engine* h_ = nullptr;
    int64_t n_train_ = 0, n_test_ = 0;
    bool computed_ = false;
    int device0_ = 0;
    // skip_test_block="lazy" / None: the test x test block is left out of compute_kernel and computed only if asked for
    bool lazy_test_block_ = false, test_block_missing_ = false;
    bool revcomp_ = false;
    std::vector<int32_t> wildcards_;
    std::vector<uint32_t> center_weights_;  // centre-weighted mode: the profile (empty: off)
    std::vector<uint64_t> weights_;      // mismatch-weighted mode: c_0..c_m (empty: off)
    std::vector<int32_t> labels_;        // fit_svm: the labels of the model at hand
    bool svr_ = false;                   // the model at hand is fit_svr's (the one model slot holds either kind)
    std::vector<int32_t> kept_tokens_;   // the call's input, kept while the test x test block is missing
    std::vector<int64_t> kept_offsets_;

    void check(int rc) const {
        if (rc == FSK_OK) return;
        std::string msg = fsk_last_error(h_);
        if (rc == FSK_EINVAL || rc == FSK_ESHORT) throw py::value_error(msg);
        throw std::runtime_error(msg);
    }
    void run_flat(const int32_t* tokens, const int64_t* offsets, int64_t n_train, int64_t n_test) {
        const bool skip = lazy_test_block_ && n_test > 0;
        if (lazy_test_block_) check(fsk_set_skip_test_block(h_, skip ? 1 : 0));
        int rc;
        {
            py::gil_scoped_release nogil;  // the reference holds the GIL for the whole call
            rc = fsk_compute(h_, tokens, offsets, n_train, n_test);
        }
        check(rc);
        n_train_ = n_train;
        n_test_ = n_test;
        computed_ = true;
        test_block_missing_ = skip;
        if (skip) {
            if (tokens != kept_tokens_.data()) {
                kept_tokens_.assign(tokens + offsets[0], tokens + offsets[n_train + n_test]);
                kept_offsets_.assign(offsets, offsets + n_train + n_test + 1);
                for (auto& o : kept_offsets_) o -= offsets[0];
            }
        } else {
            kept_tokens_.clear(); kept_tokens_.shrink_to_fit();
            kept_offsets_.clear();
        }
    }
    void run(const Flat& f, int64_t n_train, int64_t n_test) { run_flat(f.tokens.data(), f.offsets.data(), n_train, n_test); }
    // something wants cells with both sequences in the test set: the same call again, nothing left out
    void need_test_block() {
        if (!test_block_missing_) return;
        check(fsk_set_skip_test_block(h_, 0));
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = fsk_compute(h_, kept_tokens_.data(), kept_offsets_.data(), n_train_, n_test_);
        }
        check(rc);
        test_block_missing_ = false;
        kept_tokens_.clear(); kept_tokens_.shrink_to_fit();
        kept_offsets_.clear();
    }
    // device memory of the engine's first GPU (released with fsk_free_device) as a DLPack capsule of float64
    py::capsule dlpack_of(double* dev, int ndim, int64_t d0, int64_t d1) {
        auto* owner = new BlockOwner{{d0, d1}};
        auto* mt = new DLManagedTensor{};
        mt->dl_tensor.data = dev;
        mt->dl_tensor.device = DLDevice{kDLROCM, device0_};
        mt->dl_tensor.ndim = ndim;
        mt->dl_tensor.dtype = DLDataType{kDLFloat, 64, 1};
        mt->dl_tensor.shape = owner->shape;
        mt->dl_tensor.strides = nullptr;  // compact row-major
        mt->dl_tensor.byte_offset = 0;
        mt->manager_ctx = owner;
        mt->deleter = [](DLManagedTensor* t) {  // (the block outlives the FastSK object if its consumer does)
            (void)fsk_free_device(nullptr, t->dl_tensor.data);
            delete static_cast<BlockOwner*>(t->manager_ctx);
            delete t;
        };
        return py::capsule(mt, "dltensor", [](PyObject* cap) {
            if (PyCapsule_IsValid(cap, "dltensor")) {  // never consumed: ours to free
                auto* t = static_cast<DLManagedTensor*>(PyCapsule_GetPointer(cap, "dltensor"));
                if (t && t->deleter) t->deleter(t);
            }
        });
    }
    py::capsule dlpack_block(int64_t i0, int64_t i1, int64_t j0, int64_t j1) {
        if (!computed_) throw std::runtime_error("call compute_kernel or compute_train first");
        if (i1 < i0 || j1 < j0) throw py::value_error("empty block");
        if (i1 > n_train_ && j1 > n_train_) need_test_block();
        double* dev = nullptr;
        check(fsk_alloc_block_device(h_, i0, i1, j0, j1, &dev));
        return dlpack_of(dev, 2, i1 - i0, j1 - j0);
    }
    py::array_t<double> block(bool test) const {
        if (!computed_) throw std::runtime_error("call compute_kernel or compute_train first");
        const int64_t rows = test ? n_test_ : n_train_;
        py::array_t<double> out({(py::ssize_t)rows, (py::ssize_t)n_train_});
        if (rows > 0) check(test ? fsk_get_test(h_, out.mutable_data()) : fsk_get_train(h_, out.mutable_data()));
        return out;
    }
    // the reference's return type, vector<vector<double>> -> a list of lists of floats, built from the block's one host copy
    // (no vector of vectors in between; what is left is one PyFloat per cell: ~12 ns each, 8 * 10^6 of them at EP300)
    static py::list to_lists(const py::array_t<double>& a) {
        const py::ssize_t r = a.shape(0), c = a.shape(1);
        const double* p = a.data();
        py::list out(r);
        for (py::ssize_t i = 0; i < r; ++i) {
            PyObject* row = PyList_New(c);
            if (!row) throw py::error_already_set();
            for (py::ssize_t j = 0; j < c; ++j) {
                PyObject* v = PyFloat_FromDouble(p[i * c + j]);
                if (!v) { Py_DECREF(row); throw py::error_already_set(); }
                PyList_SET_ITEM(row, j, v);
            }
            PyList_SET_ITEM(out.ptr(), i, row);  // (py::list(r) holds r null slots)
        }
        return out;
    }

public:
    FastSK(int g, int m, int t, bool approx, double delta, int max_iters, bool skip_variance, int device,
           const std::string& path, py::object seed, py::object skip_test_block, py::object devices,
           const std::string& collective, int deadline_ms, py::object revcomp, py::object weights, py::object max_mismatches,
           py::object wildcards, py::object center_weights) {
        fsk_config c{};
        parse_weights(g, m, weights, max_mismatches);  // (host only: ValueError before any device call)
        parse_wildcards(wildcards);
        parse_center_weights(center_weights);
        if (!weights_.empty() && approx)
            throw py::value_error("weights= / max_mismatches= with approx=True: a sample of combinations under signed level coefficients estimates nothing");
        if (!weights_.empty() && !devices.is_none())
            throw py::value_error("weights= / max_mismatches= with devices=[...]: a group of engines does not run the levels");
        if (skip_test_block.is_none()) lazy_test_block_ = true;
        else if (py::isinstance<py::str>(skip_test_block)) {
            if (skip_test_block.cast<std::string>() != "lazy") throw py::value_error("skip_test_block must be False, True or \"lazy\"");
            lazy_test_block_ = true;
        }
        c.skip_test_block = lazy_test_block_ ? 0 : (skip_test_block.cast<bool>() ? 1 : 0);
        c.g = g; c.m = m; c.t = t; c.approx = approx; c.delta = delta; c.max_iters = max_iters;
        c.skip_variance = skip_variance; c.device = device; c.path = parse_path(path);
        c.collective = parse_collective(collective);
        c.deadline_ms = deadline_ms;
        int rc;
        if (devices.is_none()) {
            device0_ = device;
            rc = fsk_create(&c, &h_);
        } else {
            const std::vector<int32_t> devs = devices.cast<std::vector<int32_t>>();
            if (devs.empty()) throw py::value_error("devices must list at least one GPU");
            device0_ = devs[0];
            rc = fsk_create_multi(&c, devs.data(), (int32_t)devs.size(), &h_);
        }
        if (rc != FSK_OK) {
            std::string msg = fsk_last_error(nullptr);
            if (rc == FSK_EINVAL) throw py::value_error(msg);
            throw std::runtime_error(msg);
        }
        try {
            if (!seed.is_none()) check(fsk_set_seed(h_, seed.cast<uint64_t>()));
            set_revcomp(revcomp);
            if (!wildcards_.empty()) check(fsk_set_wildcards(h_, wildcards_.data(), (int32_t)wildcards_.size()));
            if (!center_weights_.empty()) check(fsk_set_center_weights(h_, center_weights_.data(), (int32_t)center_weights_.size()));
            if (!weights_.empty()) check(fsk_set_mismatch_weights(h_, weights_.data(), (int32_t)weights_.size()));
        } catch (...) {
            fsk_destroy(h_);
            h_ = nullptr;
            throw;
        }
    }
    // weights= / max_mismatches= -> weights_ (empty: off), checked as fsk_set_mismatch_weights checks them
    void parse_weights(int g, int m, const py::object& weights, const py::object& max_mismatches) {
        weights_.clear();
        if (weights.is_none() && max_mismatches.is_none()) return;
        if (!weights.is_none() && !max_mismatches.is_none()) throw py::value_error("give weights= or max_mismatches=, not both");
        if (g <= 0 || m < 0 || m >= g) throw py::value_error("need 0 <= m < g");
        if (!max_mismatches.is_none()) {
            if (!py::isinstance<py::int_>(max_mismatches) || py::isinstance<py::bool_>(max_mismatches)) throw py::value_error("max_mismatches must be an int");
            const long long d = max_mismatches.cast<long long>();
            if (d < 0 || d > m) throw py::value_error("max_mismatches must lie in 0..m");
            for (int h = 0; h <= m; ++h) {
                const int64_t b = fsk_num_combos(g - h, m - h);
                if (b >= INT64_MAX / 2) throw py::value_error("max_mismatches: C(g-h, m-h) does not fit 64 bits");
                weights_.push_back(h <= d ? (uint64_t)b : 0);
            }
        } else {
            if (py::isinstance<py::str>(weights) || py::isinstance<py::bytes>(weights) || !py::isinstance<py::sequence>(weights))
                throw py::value_error("weights must be a sequence of m + 1 non-negative ints");
            for (auto w : weights.cast<py::sequence>()) {
                if (!py::isinstance<py::int_>(w) || py::isinstance<py::bool_>(w)) throw py::value_error("weights must be non-negative ints");
                const unsigned long long v = PyLong_AsUnsignedLongLong(w.ptr());
                if (v == (unsigned long long)-1 && PyErr_Occurred()) { PyErr_Clear(); throw py::value_error("weights must lie in 0 .. 2^64 - 1"); }
                weights_.push_back((uint64_t)v);
            }
            if ((int)weights_.size() != m + 1) { weights_.clear(); throw py::value_error("weights must hold m + 1 values"); }
        }
        if (weights_[0] < 1) { weights_.clear(); throw py::value_error("weights[0] must be at least 1: it keeps every diagonal positive"); }
        std::vector<int64_t> a(weights_.size());
        int32_t n_levels = 0;
        if (fsk_mismatch_levels(g, weights_.data(), (int32_t)weights_.size(), a.data(), &n_levels) != FSK_OK) {
            weights_.clear();
            throw py::value_error(fsk_last_error(nullptr));
        }
    }
    // center_weights= -> center_weights_ (empty: off), checked as fsk_set_center_weights checks them
    void parse_center_weights(const py::object& cw) {
        center_weights_.clear();
        if (cw.is_none() || (py::isinstance<py::bool_>(cw) && !cw.cast<bool>())) return;
        if (py::isinstance<py::str>(cw) || py::isinstance<py::bytes>(cw) || !py::isinstance<py::iterable>(cw))
            throw py::value_error("center_weights must be None or a sequence of integers");
        std::vector<uint32_t> out;
        for (auto t : cw.cast<py::iterable>()) {
            if (py::isinstance<py::bool_>(t) || !(py::isinstance<py::int_>(t) || py::hasattr(t, "__index__")))
                throw py::value_error("center_weights: weights must be integers");
            long long v = -1;
            try {
                v = py::int_(t.attr("__index__")()).cast<long long>();
            } catch (...) {
                v = -1;
            }
            if (v < 0 || v > 255) throw py::value_error("center_weights: weights must lie in 0..255");
            out.push_back((uint32_t)v);
            if (out.size() > 4096) throw py::value_error("center_weights: at most 4096 entries");
        }
        if (!out.empty() && out[0] == 0) throw py::value_error("center_weights: the first entry (the centre's weight) must be at least 1");
        center_weights_.swap(out);
    }
    // wildcards= -> wildcards_ (empty: off), checked as fsk_set_wildcards checks them
    void parse_wildcards(const py::object& wildcards) {
        wildcards_.clear();
        if (wildcards.is_none() || (py::isinstance<py::bool_>(wildcards) && !wildcards.cast<bool>())) return;
        if (py::isinstance<py::str>(wildcards) || py::isinstance<py::bytes>(wildcards) || !py::isinstance<py::iterable>(wildcards))
            throw py::value_error("wildcards must be None or a sequence of token ids");
        for (auto t : wildcards.cast<py::iterable>()) {
            if (py::isinstance<py::bool_>(t) || !(py::isinstance<py::int_>(t) || py::hasattr(t, "__index__"))) {
                wildcards_.clear();
                throw py::value_error("wildcards: token ids must be integers");
            }
            long long v = 0;
            try {
                v = py::int_(t.attr("__index__")()).cast<long long>();
            } catch (...) {
                wildcards_.clear();
                throw py::value_error("wildcards: token ids must fit 32 bits");
            }
            if (v < INT32_MIN || v > INT32_MAX) { wildcards_.clear(); throw py::value_error("wildcards: token ids must fit 32 bits"); }
            for (int32_t seen : wildcards_)
                if (seen == (int32_t)v) { wildcards_.clear(); throw py::value_error("wildcards: a token is listed twice"); }
            wildcards_.push_back((int32_t)v);
        }
    }
    // None / False: off; else a mapping {token_id: token_id} that fsk_set_complement checks (ValueError)
    void set_revcomp(const py::object& revcomp) {
        std::vector<int32_t> tokens, comps;
        if (!revcomp.is_none() && !(py::isinstance<py::bool_>(revcomp) && !revcomp.cast<bool>())) {
            if (!py::isinstance<py::dict>(revcomp)) throw py::value_error("revcomp must be None, False or a mapping {token_id: token_id}");
            for (auto kv : revcomp.cast<py::dict>()) {
                if (!py::isinstance<py::int_>(kv.first) || !py::isinstance<py::int_>(kv.second) || py::isinstance<py::bool_>(kv.first) ||
                    py::isinstance<py::bool_>(kv.second))
                    throw py::value_error("revcomp: token ids must be integers");
                const long long a = kv.first.cast<long long>(), b = kv.second.cast<long long>();
                if (a < INT32_MIN || a > INT32_MAX || b < INT32_MIN || b > INT32_MAX) throw py::value_error("revcomp: token ids must fit 32 bits");
                tokens.push_back((int32_t)a);
                comps.push_back((int32_t)b);
            }
        }
        check(fsk_set_complement(h_, tokens.data(), comps.data(), (int32_t)tokens.size()));
        revcomp_ = !tokens.empty();
    }
    ~FastSK() { fsk_destroy(h_); }
    FastSK(const FastSK&) = delete;
    FastSK& operator=(const FastSK&) = delete;

    // FastSK::compute_kernel, fastsk.cpp:30-118. Xtrain / Xtest: lists of lists of ints as the reference takes them — or
    // tuples, int arrays per sequence, one 2-D integer array (fixed-length sequences) — see Flat::add
    void compute_kernel(py::object Xtrain, py::object Xtest) {
        Flat f;
        const size_t ntr = f.add(Xtrain), nte = f.add(Xtest);
        if (ntr == 0 || nte == 0) throw py::value_error("Xtrain and Xtest must be non-empty (use compute_train for train only)");
        run(f, (int64_t)ntr, (int64_t)nte);
    }
    // Additive: ragged sequences already flattened (tokens + offsets, train rows first), e.g.
    // from FastaUtility.read_packed
    void compute_kernel_flat(py::array_t<int32_t, py::array::c_style> tokens, py::array_t<int64_t, py::array::c_style> offsets,
                             int64_t n_train) {
        if (tokens.ndim() != 1 || offsets.ndim() != 1 || offsets.shape(0) < 2) throw py::value_error("expected 1-D tokens and offsets");
        const int64_t n = (int64_t)offsets.shape(0) - 1;
        if (n_train <= 0 || n_train > n) throw py::value_error("n_train out of range");
        if (offsets.data()[0] != 0 || offsets.data()[n] != (int64_t)tokens.shape(0)) throw py::value_error("offsets must start at 0 and end at len(tokens)");
        run_flat(tokens.data(), offsets.data(), n_train, n - n_train);
    }
    // FastSK::compute_train, fastsk.cpp:120-188
    void compute_train(py::object Xtrain) {
        Flat f;
        const size_t ntr = f.add(Xtrain);
        if (ntr == 0) throw py::value_error("Xtrain must be non-empty");
        run(f, (int64_t)ntr, 0);
    }
    py::list get_train_kernel() const { return to_lists(block(false)); }  // fastsk.cpp:190-200
    py::list get_test_kernel() const { return to_lists(block(true)); }    // fastsk.cpp:202-217
    py::array_t<double> get_train_kernel_np() const { return block(false); }
    py::array_t<double> get_test_kernel_np() const { return block(true); }
    std::vector<double> get_stdevs() const {  // fastsk.cpp:219-221
        int32_t n = 0;
        check(fsk_get_stdevs(h_, nullptr, 0, &n));
        std::vector<double> v((size_t)n);
        if (n) check(fsk_get_stdevs(h_, v.data(), n, &n));
        return v;
    }
    void save_kernel(const std::string& path) {  // fastsk.cpp:223-237 (the whole N x N matrix)
        need_test_block();
        check(fsk_save_kernel(h_, path.c_str()));
    }
    // the same blocks as device-resident DLPack capsules (float64, row-major, on the engine's first GPU):
    // torch.from_dlpack(f.get_train_kernel_dlpack()) keeps the kernel matrix on the GPU for the SVM stage
    py::capsule get_train_kernel_dlpack() { return dlpack_block(0, n_train_, 0, n_train_); }
    py::capsule get_test_kernel_dlpack() { return dlpack_block(n_train_, n_train_ + n_test_, 0, n_train_); }
    py::capsule get_block_dlpack(int64_t i0, int64_t i1, int64_t j0, int64_t j1) { return dlpack_block(i0, i1, j0, j1); }
    void set_combo_order(std::vector<int32_t> order) {
        // a result whose test x test block is still to come belongs to the OLD order: complete it first, so that
        // every block of one compute_kernel call comes from one set of combos
        need_test_block();
        check(fsk_set_combo_order(h_, order.data(), (int32_t)order.size()));
    }
    py::array_t<double> get_block(int64_t i0, int64_t i1, int64_t j0, int64_t j1) {
        if (i1 < i0 || j1 < j0) throw py::value_error("empty block");
        if (i1 > n_train_ && j1 > n_train_) need_test_block();
        py::array_t<double> out({(py::ssize_t)(i1 - i0), (py::ssize_t)(j1 - j0)});
        check(fsk_get_block(h_, i0, i1, j0, j1, out.mutable_data()));
        return out;
    }
    py::array_t<uint64_t> get_counts_np() {
        if (!computed_) throw std::runtime_error("call compute_kernel or compute_train first");
        need_test_block();
        const int64_t N = n_train_ + n_test_;
        py::array_t<uint64_t> out((py::ssize_t)(N * (N + 1) / 2));
        check(fsk_get_counts(h_, out.mutable_data()));
        return out;
    }
    // ---- additive: the raw integer kernel without copying the triangle out (exact and skip-variance modes).
    // The reference has no such getter (its K is normalised in place, fastsk_kernel.cpp:96-103); these are what a
    // caller uses to check a 100k-sequence result, whose triangle is 40 GB.
    // (sum, xor of cell * (index | 1)) mod 2^64 over the integer cells of rows [row_begin, row_end): fsk_counts_digest
    py::tuple counts_digest(int64_t row_begin, int64_t row_end) {
        if (!computed_) throw std::runtime_error("call compute_kernel or compute_train first");
        const int64_t N = n_train_ + n_test_;
        if (row_end < 0) row_end = N;
        if (row_end > n_train_ + 1) need_test_block();  // (row n_train holds one test x test cell, its diagonal, always computed)
        uint64_t d[2] = {0, 0};
        check(fsk_counts_digest(h_, row_begin, row_end, d));
        return py::make_tuple(py::int_(d[0]), py::int_(d[1]));
    }
    py::array_t<uint64_t> get_counts_block(int64_t i0, int64_t i1, int64_t j0, int64_t j1) {
        if (!computed_) throw std::runtime_error("call compute_kernel or compute_train first");
        if (i1 < i0 || j1 < j0) throw py::value_error("empty block");
        if (i1 > n_train_ && j1 > n_train_) need_test_block();
        py::array_t<uint64_t> out({(py::ssize_t)(i1 - i0), (py::ssize_t)(j1 - j0)});
        check(fsk_get_counts_block(h_, i0, i1, j0, j1, out.mutable_data()));
        return out;
    }
    // scattered cells (rows[q], cols[q]) of the symmetric integer matrix: tri_access of arbitrary pairs, shared.cpp:97-117
    py::array_t<uint64_t> get_counts_cells(py::array_t<int64_t, py::array::c_style | py::array::forcecast> rows,
                                           py::array_t<int64_t, py::array::c_style | py::array::forcecast> cols) {
        if (!computed_) throw std::runtime_error("call compute_kernel or compute_train first");
        if (rows.ndim() != 1 || cols.ndim() != 1 || rows.shape(0) != cols.shape(0)) throw py::value_error("rows and cols must be 1-D and of equal length");
        const int64_t n = (int64_t)rows.shape(0);
        if (test_block_missing_)
            for (int64_t q = 0; q < n; ++q)
                if (rows.data()[q] >= n_train_ && cols.data()[q] >= n_train_ && rows.data()[q] != cols.data()[q]) { need_test_block(); break; }
        py::array_t<uint64_t> out((py::ssize_t)n);
        check(fsk_get_counts_cells(h_, rows.data(), cols.data(), n, out.mutable_data()));
        return out;
    }
    // the reference's K itself — the whole normalised lower triangle, cell (i, j <= i) at i(i+1)/2 + j
    // (fastsk_kernel.cpp:96-103) — resident on the GPU as a 1-D float64 DLPack capsule
    py::capsule get_triangle_dlpack() {
        if (!computed_) throw std::runtime_error("call compute_kernel or compute_train first");
        need_test_block();
        double* dev = nullptr;
        check(fsk_alloc_triangle_device(h_, &dev));
        const int64_t N = n_train_ + n_test_;
        return dlpack_of(dev, 1, N * (N + 1) / 2, 1);
    }
    py::dict stats() const {
        fsk_stats s;
        check(fsk_get_stats(h_, &s));
        py::dict d;
        d["n_seq"] = s.n_seq; d["n_feat"] = s.n_feat; d["n_pairs"] = s.n_pairs; d["alphabet"] = s.alphabet;
        d["bits_per_symbol"] = s.bits_per_symbol; d["key_space"] = s.key_space;
        d["path_used"] = s.path_used == FSK_PATH_DENSE ? "dense" : "sparse";
        d["n_combos_total"] = s.n_combos_total; d["combos_done"] = s.combos_done;
        d["cell_updates"] = s.cell_updates; d["launches"] = s.launches;
        d["test_block_computed"] = computed_ && !test_block_missing_;
        d["revcomp"] = revcomp_;
        {
            py::list wl;
            for (int32_t v : wildcards_) wl.append(v);
            d["wildcards"] = wl;
        }
        if (center_weights_.empty()) d["center_weights"] = py::none();
        else {
            py::list cl;
            for (uint32_t v : center_weights_) cl.append(v);
            d["center_weights"] = cl;
        }
        if (weights_.empty()) d["weights"] = py::none();
        else {
            py::list w;
            for (uint64_t v : weights_) w.append(py::int_(v));
            d["weights"] = w;
        }
        d["mismatch_levels"] = mismatch_info()["levels"];
        fsk_multi_info mi;
        check(fsk_get_multi_info(h_, &mi));
        py::list devs;
        for (int r = 0; r < mi.ndev; ++r) devs.append(mi.devices[r]);
        if (mi.ndev == 0) devs.append(device0_);
        d["devices"] = devs;
        d["collective"] = mi.ndev == 0 ? "none" : mi.collective == FSK_COLL_RCCL ? "rccl" : "p2p";
        d["comm_ranks"] = mi.comm_ranks; d["exchange_bands"] = mi.bands; d["exchange_int32"] = (bool)mi.narrow;
        return d;
    }
    // what the last compute did in mismatch-weighted mode (fsk_get_mismatch_info): n_levels = 0 with the mode off
    py::dict mismatch_info() const {
        int32_t n = 0;
        check(fsk_get_mismatch_info(h_, &n, nullptr, nullptr, 0));
        std::vector<int64_t> a((size_t)n);
        std::vector<int32_t> paths((size_t)n);
        std::vector<double> ms((size_t)n), fold((size_t)n);
        if (n) {
            check(fsk_get_mismatch_info(h_, &n, a.data(), paths.data(), n));
            check(fsk_get_mismatch_times(h_, ms.data(), fold.data(), n));
        }
        py::list levels, coeff;
        for (int32_t j = 0; j < n; ++j) {
            coeff.append(a[(size_t)j]);
            if (a[(size_t)j] == 0) continue;
            py::dict lv;
            lv["m"] = j; lv["a"] = a[(size_t)j];
            lv["path"] = paths[(size_t)j] == FSK_PATH_DENSE ? "dense" : "sparse";
            lv["ms"] = ms[(size_t)j]; lv["fold_ms"] = fold[(size_t)j];
            levels.append(lv);
        }
        py::dict d;
        d["n_levels"] = n; d["a"] = coeff; d["levels"] = levels;
        return d;
    }
    // ---- additive: the SVM stage on the resident triangle (fsk_svm_train / fsk_svm_decision). fit() / score() stay the
    // reference's stubs; these train and score on the result compute_kernel / compute_train has left on the device.
    // kernel_type: "fastsk" — the gapped-k-mer kernel itself; "linear" — its rows as feature vectors, the reference's default
    // (fastsk.cpp:239-291) through the rows kernel K2 (fsk_rows_build); "rbf" is not built
    static int32_t parse_kernel_type(const std::string& kt) {
        if (kt == "fastsk") return FSK_SVM_KERNEL_RESULT;
        if (kt == "linear") return FSK_SVM_KERNEL_ROWS;
        if (kt == "rbf") throw py::value_error("kernel_type=\"rbf\" is not built: a device exp cannot be restated bit for bit; use \"fastsk\" or \"linear\"");
        throw py::value_error("kernel_type must be \"fastsk\" or \"linear\"");
    }
    // class_weight: None, "balanced" (n / (2 n_pos), n / (2 n_neg), from all the labels, once), a pair (w_pos, w_neg) or a dict
    // keyed by 1 / -1 (fastsk_amd.class_weights). probability=True: Platt's sigmoid on the out-of-fold decision values of
    // stratified_folds(labels, calibration_folds, seed) (fsk_svm_calibrate); predict_proba_np then gives P(y = +1).
    static std::pair<double, double> parse_class_weight(const py::object& labels, const py::object& spec) {
        return py::module_::import("fastsk_amd._native").attr("class_weights")(labels, spec).cast<std::pair<double, double>>();
    }
    static py::dict info_dict(const fsk_svm_info& s, const std::string& kernel_type) {
        py::dict d;
        d["iterations"] = s.iterations; d["gap"] = s.gap; d["objective"] = s.objective; d["n_sv"] = s.n_sv; d["n_bsv"] = s.n_bsv;
        d["converged"] = (bool)s.converged; d["form"] = s.form == 1 ? "workgroup" : "two-launch"; d["launches"] = s.launches;
        d["ms"] = s.ms; d["kernel_type"] = kernel_type;
        return d;
    }
    py::dict fit_svm(py::array_t<int32_t, py::array::c_style | py::array::forcecast> labels, double C, double eps, int64_t max_iter,
                     const std::string& kernel_type, py::object class_weight, bool probability, int32_t calibration_folds, uint64_t seed) {
        const int32_t kind = parse_kernel_type(kernel_type);  // (ValueError before any device call)
        if (!computed_) throw std::runtime_error("call compute_kernel or compute_train first");
        if (labels.ndim() != 1) throw py::value_error("labels must be 1-D, one of -1 / +1 per training sequence");
        const std::pair<double, double> w = parse_class_weight(labels, class_weight);
        py::array_t<int32_t, py::array::c_style | py::array::forcecast> fold;
        if (probability) fold = py::module_::import("fastsk_amd._native").attr("stratified_folds")(labels, calibration_folds, seed);
        check(fsk_svm_set_kernel(h_, kind));
        check(fsk_svm_set_class_weights(h_, w.first, w.second));
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = fsk_svm_train(h_, labels.data(), (int64_t)labels.shape(0), C, eps, max_iter);
        }
        check(rc);
        labels_.assign(labels.data(), labels.data() + labels.shape(0));
        svr_ = false;
        fsk_svm_info s;
        check(fsk_svm_get_model(h_, nullptr, nullptr, &s));
        py::dict d = info_dict(s, kernel_type);
        d["class_weight"] = py::make_tuple(w.first, w.second);
        if (probability) {
            if (fold.ndim() != 1 || fold.shape(0) != labels.shape(0)) throw py::value_error("one fold id per label");
            {
                py::gil_scoped_release nogil;
                rc = fsk_svm_calibrate(h_, fold.data(), calibration_folds);
            }
            check(rc);
            fsk_svm_platt_info q;
            check(fsk_svm_get_calibration(h_, nullptr, &q));
            py::dict pl;
            pl["A"] = q.A; pl["B"] = q.B; pl["iterations"] = q.iterations; pl["status"] = q.status; pl["n_folds"] = q.n_folds;
            pl["form"] = q.form == 1 ? "workgroup" : "two-launch"; pl["launches"] = q.launches; pl["ms"] = q.ms;
            d["platt"] = pl;
        }
        return d;
    }
    // cells [i0, i1) x [j0, j1) of the rows kernel (built if it is not there): L when raw, else K2. Only cells of the result
    // with a train column are read: nothing here asks for the test x test block.
    py::array_t<double> get_rows_kernel_block_np(int64_t i0, int64_t i1, int64_t j0, int64_t j1, bool raw) {
        if (!computed_) throw std::runtime_error("call compute_kernel or compute_train first");
        if (i1 < i0 || j1 < j0) throw py::value_error("empty block");
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = fsk_rows_build(h_);
        }
        check(rc);
        py::array_t<double> out({(py::ssize_t)(i1 - i0), (py::ssize_t)(j1 - j0)});
        check(fsk_rows_get_block(h_, i0, i1, j0, j1, raw ? 1 : 0, out.mutable_data()));
        return out;
    }
    py::dict rows_kernel_info() const {
        fsk_rows_info s;
        check(fsk_rows_get_info(h_, &s));
        py::dict d;
        d["n_train"] = s.n_train; d["n_seq"] = s.n_seq; d["tile"] = s.tile; d["panel"] = s.panel; d["tiles"] = s.tiles; d["builds"] = s.builds;
        d["scratch_bytes"] = s.scratch_bytes; d["resident_bytes"] = s.resident_bytes; d["ms_scratch"] = s.ms_scratch; d["ms_product"] = s.ms_product;
        return d;
    }
    // cross-validation of the C-SVC over folds and values of C, every problem solved side by side (fsk_svm_cv). folds: an int
    // (fastsk_amd.stratified_folds(labels, folds, seed)) or an array of fold ids 0..F-1. best_C: the C of the highest
    // out-of-fold AUC, the smallest of equals; refit=True then trains the model of fit_svm(labels, C=best_C, eps).
    py::dict cross_validate_svm(py::array_t<int32_t, py::array::c_style | py::array::forcecast> labels,
                                py::array_t<double, py::array::c_style | py::array::forcecast> Cs, py::object folds, double eps,
                                int64_t max_iter, uint64_t seed, bool refit, const std::string& kernel_type, py::object class_weight) {
        const int32_t kind = parse_kernel_type(kernel_type);  // (ValueError before any device call)
        if (!computed_) throw std::runtime_error("call compute_kernel or compute_train first");
        if (labels.ndim() != 1) throw py::value_error("labels must be 1-D, one of -1 / +1 per training sequence");
        if (Cs.ndim() != 1) throw py::value_error("Cs must be 1-D");
        const std::pair<double, double> w = parse_class_weight(labels, class_weight);
        py::array_t<int32_t, py::array::c_style | py::array::forcecast> fold;
        int32_t n_folds = 0;
        if (py::isinstance<py::int_>(folds) && !py::isinstance<py::bool_>(folds)) {
            n_folds = folds.cast<int32_t>();
            fold = py::module_::import("fastsk_amd._native").attr("stratified_folds")(labels, folds, seed);
        } else {
            fold = folds.cast<py::array_t<int32_t, py::array::c_style | py::array::forcecast>>();
            if (fold.ndim() != 1 || fold.shape(0) != labels.shape(0)) throw py::value_error("folds must be an int or one fold id per label");
            for (py::ssize_t t = 0; t < fold.shape(0); ++t) n_folds = std::max(n_folds, fold.data()[t] + 1);
        }
        const int64_t n = (int64_t)labels.shape(0);
        const int32_t n_C = (int32_t)Cs.shape(0);
        check(fsk_svm_set_kernel(h_, kind));
        check(fsk_svm_set_class_weights(h_, w.first, w.second));
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = fsk_svm_cv(h_, labels.data(), n, fold.data(), n_folds, Cs.data(), n_C, eps, max_iter);
        }
        check(rc);
        const int64_t P = (int64_t)n_C * n_folds;
        py::array_t<double> oof({(py::ssize_t)n_C, (py::ssize_t)n}), auc((py::ssize_t)n_C), acc((py::ssize_t)n_C);
        std::vector<fsk_svm_cv_score> scores((size_t)n_C);
        std::vector<fsk_svm_cv_problem> probs((size_t)P);
        fsk_svm_cv_info info;
        check(fsk_svm_cv_get(h_, oof.mutable_data(), scores.data(), probs.data(), &info));
        int32_t best = 0;
        for (int32_t c = 0; c < n_C; ++c) {
            auc.mutable_data()[c] = scores[(size_t)c].auc;
            acc.mutable_data()[c] = scores[(size_t)c].accuracy;
            const fsk_svm_cv_score &x = scores[(size_t)c], &b = scores[(size_t)best];
            if (x.auc > b.auc || (x.auc == b.auc && x.C < b.C)) best = c;
        }
        py::list problems;
        for (const fsk_svm_cv_problem& q : probs) {
            py::dict d;
            d["n_rows"] = q.n_rows; d["iterations"] = q.iterations; d["converged"] = (bool)q.converged; d["gap"] = q.gap;
            d["objective"] = q.objective; d["rho"] = q.rho; d["n_sv"] = q.n_sv; d["n_bsv"] = q.n_bsv; d["C"] = q.C; d["fold"] = q.fold;
            problems.append(d);
        }
        py::dict d;
        d["decision"] = oof; d["auc"] = auc; d["accuracy"] = acc; d["problems"] = problems;
        d["form"] = info.form == 1 ? "workgroup" : "two-launch"; d["launches"] = info.launches; d["ms"] = info.ms;
        d["fold"] = fold; d["best_C"] = scores[(size_t)best].C; d["kernel_type"] = kernel_type;
        d["class_weight"] = py::make_tuple(w.first, w.second);
        if (refit) d["refit"] = fit_svm(labels, scores[(size_t)best].C, eps, max_iter, kernel_type, py::make_tuple(w.first, w.second), false, 5, 0);
        return d;
    }
    // ---- epsilon-SVR on the resident triangle (fsk_svr_train): real-valued targets; the model takes the one model slot, so
    // get_dual_coef_np (alpha - alpha*), get_intercept (-rho), decision_function_* and predict_* then speak of it, and
    // predict_proba_np raises RuntimeError. Class weights do not apply to a regression.
    py::dict fit_svr(py::array_t<double, py::array::c_style | py::array::forcecast> targets, double C, double epsilon, double eps, int64_t max_iter,
                     const std::string& kernel_type) {
        const int32_t kind = parse_kernel_type(kernel_type);  // (ValueError before any device call)
        if (!computed_) throw std::runtime_error("call compute_kernel or compute_train first");
        if (targets.ndim() != 1) throw py::value_error("targets must be 1-D, one real number per training sequence");
        check(fsk_svm_set_kernel(h_, kind));
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = fsk_svr_train(h_, targets.data(), (int64_t)targets.shape(0), C, epsilon, eps, max_iter);
        }
        check(rc);
        svr_ = true;
        fsk_svm_info s;
        check(fsk_svr_get_model(h_, nullptr, nullptr, nullptr, &s));
        py::dict d = info_dict(s, kernel_type);
        d["epsilon"] = epsilon;
        return d;
    }
    // cross-validation of the SVR over folds and the grid Cs x epsilons, every problem side by side (fsk_svr_cv). folds: an int
    // (fastsk_amd.kfold(n, folds, seed)) or an array of fold ids. best_C, best_epsilon: the grid point of the smallest
    // out-of-fold mse, the lowest index (c n_eps + q) among equals; refit=True then trains fit_svr there.
    py::dict cross_validate_svr(py::array_t<double, py::array::c_style | py::array::forcecast> targets,
                                py::array_t<double, py::array::c_style | py::array::forcecast> Cs,
                                py::array_t<double, py::array::c_style | py::array::forcecast> epsilons, py::object folds, uint64_t seed, double eps,
                                int64_t max_iter, const std::string& kernel_type, bool refit) {
        const int32_t kind = parse_kernel_type(kernel_type);
        if (!computed_) throw std::runtime_error("call compute_kernel or compute_train first");
        if (targets.ndim() != 1) throw py::value_error("targets must be 1-D, one real number per training sequence");
        if (Cs.ndim() != 1 || epsilons.ndim() != 1) throw py::value_error("Cs and epsilons must be 1-D");
        const int64_t n = (int64_t)targets.shape(0);
        py::array_t<int32_t, py::array::c_style | py::array::forcecast> fold;
        int32_t n_folds = 0;
        if (py::isinstance<py::int_>(folds) && !py::isinstance<py::bool_>(folds)) {
            n_folds = folds.cast<int32_t>();
            fold = py::module_::import("fastsk_amd._native").attr("kfold")(n, folds, seed);
        } else {
            fold = folds.cast<py::array_t<int32_t, py::array::c_style | py::array::forcecast>>();
            if (fold.ndim() != 1 || fold.shape(0) != targets.shape(0)) throw py::value_error("folds must be an int or one fold id per target");
            for (py::ssize_t t = 0; t < fold.shape(0); ++t) n_folds = std::max(n_folds, fold.data()[t] + 1);
        }
        const int32_t n_C = (int32_t)Cs.shape(0), n_E = (int32_t)epsilons.shape(0);
        check(fsk_svm_set_kernel(h_, kind));
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = fsk_svr_cv(h_, targets.data(), n, fold.data(), n_folds, Cs.data(), n_C, epsilons.data(), n_E, eps, max_iter);
        }
        check(rc);
        const int64_t nG = (int64_t)n_C * n_E;
        py::array_t<double> oof({(py::ssize_t)n_C, (py::ssize_t)n_E, (py::ssize_t)n});
        py::array_t<double> mse({(py::ssize_t)n_C, (py::ssize_t)n_E}), mae({(py::ssize_t)n_C, (py::ssize_t)n_E}), r2({(py::ssize_t)n_C, (py::ssize_t)n_E}),
            r({(py::ssize_t)n_C, (py::ssize_t)n_E});
        std::vector<fsk_svr_cv_score> scores((size_t)nG);
        std::vector<fsk_svm_cv_problem> probs((size_t)(nG * n_folds));
        fsk_svm_cv_info info;
        check(fsk_svr_cv_get(h_, oof.mutable_data(), scores.data(), probs.data(), &info));
        int64_t best = 0;
        for (int64_t g = 0; g < nG; ++g) {
            const fsk_svr_cv_score& x = scores[(size_t)g];
            mse.mutable_data()[g] = x.mse; mae.mutable_data()[g] = x.mae; r2.mutable_data()[g] = x.r2; r.mutable_data()[g] = x.r;
            if (x.mse < scores[(size_t)best].mse) best = g;  // (the lowest index among equals)
        }
        py::list problems;
        for (const fsk_svm_cv_problem& q : probs) {
            py::dict d;
            d["n_rows"] = q.n_rows; d["iterations"] = q.iterations; d["converged"] = (bool)q.converged; d["gap"] = q.gap;
            d["objective"] = q.objective; d["rho"] = q.rho; d["n_sv"] = q.n_sv; d["n_bsv"] = q.n_bsv; d["C"] = q.C;
            d["epsilon"] = q.reserved[0]; d["fold"] = q.fold;
            problems.append(d);
        }
        py::dict inf;
        inf["form"] = info.form == 1 ? "workgroup" : "two-launch"; inf["launches"] = info.launches; inf["ms"] = info.ms;
        inf["n"] = info.n; inf["n_folds"] = info.n_folds; inf["n_C"] = info.n_C; inf["n_eps"] = info.reserved0; inf["kernel_type"] = kernel_type;
        py::dict d;
        d["mse"] = mse; d["mae"] = mae; d["r2"] = r2; d["r"] = r; d["oof"] = oof; d["problems"] = problems; d["info"] = inf; d["fold"] = fold;
        d["best_C"] = scores[(size_t)best].C; d["best_epsilon"] = scores[(size_t)best].epsilon;
        if (refit) d["refit"] = fit_svr(targets, scores[(size_t)best].C, scores[(size_t)best].epsilon, eps, max_iter, kernel_type);
        else d["refit"] = py::none();
        return d;
    }
    // ---- multi-class C-SVC, one-vs-one (fsk_svm_train_multiclass): labels are any integers, the k (k - 1) / 2 pairs of classes
    // are solved side by side in one batch; the model takes the one model slot. decision_function_np then returns [rows, P],
    // predict_class_np the voted labels; get_dual_coef_np and get_intercept raise RuntimeError naming the model, and so does
    // predict_proba_np until the model is calibrated (probability=True). class_weight: None, "balanced" (n / (k count_c)) or a dict keyed
    // by label (fastsk_amd._native.multiclass_weights).
    using WeightArray = py::array_t<double, py::array::c_style | py::array::forcecast>;
    static bool parse_multiclass_weight(const py::object& labels, const py::object& spec, WeightArray* w) {
        py::object r = py::module_::import("fastsk_amd._native").attr("multiclass_weights")(labels, spec);
        if (r.is_none()) return false;
        *w = r.cast<WeightArray>();
        return true;
    }
    static py::dict pair_dict(int32_t a, int32_t b, int64_t n_rows, int64_t iterations, bool converged, double gap, double objective, double rho,
                              int64_t n_sv, int64_t n_bsv) {
        py::dict d;
        d["class_a"] = a; d["class_b"] = b; d["n_rows"] = n_rows; d["iterations"] = iterations; d["converged"] = converged; d["gap"] = gap;
        d["objective"] = objective; d["rho"] = rho; d["n_sv"] = n_sv; d["n_bsv"] = n_bsv;
        return d;
    }
    // probability=True: a Platt sigmoid a pair on the out-of-fold pair decisions of stratified_folds(labels, calibration_folds,
    // seed) (fsk_svm_multiclass_calibrate); predict_proba_np then gives [rows, k], predict_class_np(rule="proba") its argmax.
    py::dict fit_svm_multiclass(py::array_t<int32_t, py::array::c_style | py::array::forcecast> labels, double C, double eps, int64_t max_iter,
                                const std::string& kernel_type, py::object class_weight, bool probability, int32_t calibration_folds,
                                uint64_t seed) {
        const int32_t kind = parse_kernel_type(kernel_type);  // (ValueError before any device call)
        if (!computed_) throw std::runtime_error("call compute_kernel or compute_train first");
        if (labels.ndim() != 1) throw py::value_error("labels must be 1-D, one integer per training sequence");
        WeightArray w;
        const bool weighted = parse_multiclass_weight(labels, class_weight, &w);
        py::array_t<int32_t, py::array::c_style | py::array::forcecast> fold;
        if (probability) fold = py::module_::import("fastsk_amd._native").attr("stratified_folds")(labels, calibration_folds, seed);
        check(fsk_svm_set_kernel(h_, kind));
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = fsk_svm_train_multiclass(h_, labels.data(), (int64_t)labels.shape(0), C, weighted ? w.data() : nullptr, eps, max_iter);
        }
        check(rc);
        svr_ = false;
        labels_.clear();
        fsk_svm_multiclass_info mi;
        check(fsk_svm_multiclass_get_model(h_, nullptr, nullptr, nullptr, &mi));
        py::array_t<int32_t> classes((py::ssize_t)mi.k);
        std::vector<fsk_svm_multiclass_pair> pairs((size_t)mi.n_pairs);
        check(fsk_svm_multiclass_get_model(h_, classes.mutable_data(), pairs.data(), nullptr, &mi));
        py::list pl;
        bool converged = true;
        for (const fsk_svm_multiclass_pair& q : pairs) {
            pl.append(pair_dict(q.class_a, q.class_b, q.n_rows, q.iterations, (bool)q.converged, q.gap, q.objective, q.rho, q.n_sv, q.n_bsv));
            converged = converged && q.converged;
        }
        py::dict d;
        d["classes"] = classes; d["pairs"] = pl; d["k"] = mi.k; d["n_pairs"] = mi.n_pairs; d["n_sv"] = mi.n_sv; d["converged"] = converged;
        d["form"] = mi.form == 1 ? "workgroup" : "two-launch"; d["launches"] = mi.launches; d["ms"] = mi.ms; d["kernel_type"] = kernel_type;
        if (weighted) d["class_weight"] = w; else d["class_weight"] = py::none();
        if (probability) {
            if (fold.ndim() != 1 || fold.shape(0) != labels.shape(0)) throw py::value_error("one fold id per label");
            {
                py::gil_scoped_release nogil;
                rc = fsk_svm_multiclass_calibrate(h_, fold.data(), calibration_folds);
            }
            check(rc);
            std::vector<fsk_svm_platt_info> fits((size_t)mi.n_pairs);
            check(fsk_svm_multiclass_get_calibration(h_, nullptr, fits.data()));
            py::list per_pair;
            for (const fsk_svm_platt_info& q : fits) {
                py::dict one;
                one["A"] = q.A; one["B"] = q.B; one["iterations"] = q.iterations; one["status"] = q.status;
                per_pair.append(one);
            }
            const fsk_svm_platt_info& q = fits[0];  // (what belongs to the whole call is in every fit)
            py::dict platt;
            platt["pairs"] = per_pair; platt["n_folds"] = q.n_folds; platt["form"] = q.form == 1 ? "workgroup" : "two-launch";
            platt["launches"] = q.launches; platt["ms"] = q.ms;
            d["platt"] = platt;
        }
        return d;
    }
    // the label of the test (or train) rows under the model of fit_svm_multiclass. rule="vote": LIBSVM's vote, the lowest class
    // among equal vote counts (svm_predict). rule="proba": the class of the largest coupled probability, the lowest among equals
    // (svm_predict_probability's label; needs probability=True).
    py::array_t<int32_t> predict_class_np(const std::string& which, const std::string& rule) const {
        if (rule != "vote" && rule != "proba") throw py::value_error("rule must be 'vote' or 'proba'");
        int64_t r0, r1;
        decision_rows(which, &r0, &r1);
        py::array_t<int32_t> out((py::ssize_t)(r1 - r0));
        if (rule == "proba") check(fsk_svm_multiclass_proba(h_, r0, r1, nullptr, out.mutable_data(), nullptr));
        else check(fsk_svm_multiclass_decision(h_, r0, r1, nullptr, out.mutable_data()));
        return out;
    }
    // cross-validation of the multi-class C-SVC over folds and values of C, every (C, fold, pair) problem in one batch
    // (fsk_svm_multiclass_cv). folds as for cross_validate_svm. best_C: the C of the highest out-of-fold accuracy, the smallest
    // of equals (there is no AUC for more than two classes); refit=True then trains fit_svm_multiclass(labels, C=best_C).
    py::dict cross_validate_svm_multiclass(py::array_t<int32_t, py::array::c_style | py::array::forcecast> labels,
                                           py::array_t<double, py::array::c_style | py::array::forcecast> Cs, py::object folds, double eps,
                                           int64_t max_iter, uint64_t seed, bool refit, const std::string& kernel_type, py::object class_weight,
                                           bool probability, int32_t calibration_folds) {
        const int32_t kind = parse_kernel_type(kernel_type);  // (ValueError before any device call)
        if (!computed_) throw std::runtime_error("call compute_kernel or compute_train first");
        if (labels.ndim() != 1) throw py::value_error("labels must be 1-D, one integer per training sequence");
        if (Cs.ndim() != 1) throw py::value_error("Cs must be 1-D");
        WeightArray w;
        const bool weighted = parse_multiclass_weight(labels, class_weight, &w);
        py::array_t<int32_t, py::array::c_style | py::array::forcecast> fold;
        int32_t n_folds = 0;
        if (py::isinstance<py::int_>(folds) && !py::isinstance<py::bool_>(folds)) {
            n_folds = folds.cast<int32_t>();
            fold = py::module_::import("fastsk_amd._native").attr("stratified_folds")(labels, folds, seed);
        } else {
            fold = folds.cast<py::array_t<int32_t, py::array::c_style | py::array::forcecast>>();
            if (fold.ndim() != 1 || fold.shape(0) != labels.shape(0)) throw py::value_error("folds must be an int or one fold id per label");
            for (py::ssize_t t = 0; t < fold.shape(0); ++t) n_folds = std::max(n_folds, fold.data()[t] + 1);
        }
        const int64_t n = (int64_t)labels.shape(0);
        const int32_t n_C = (int32_t)Cs.shape(0);
        check(fsk_svm_set_kernel(h_, kind));
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = fsk_svm_multiclass_cv(h_, labels.data(), n, fold.data(), n_folds, Cs.data(), n_C, weighted ? w.data() : nullptr, eps, max_iter);
        }
        check(rc);
        fsk_svm_cv_info info;
        check(fsk_svm_multiclass_cv_get(h_, nullptr, nullptr, nullptr, &info));
        const int64_t k = info.reserved0, total = (int64_t)n_C * n_folds * (k * (k - 1) / 2);
        py::array_t<int32_t> pred({(py::ssize_t)n_C, (py::ssize_t)n});
        py::array_t<double> acc((py::ssize_t)n_C);
        std::vector<fsk_svm_cv_score> scores((size_t)n_C);
        std::vector<fsk_svm_cv_problem> probs((size_t)total);
        check(fsk_svm_multiclass_cv_get(h_, pred.mutable_data(), scores.data(), probs.data(), &info));
        int32_t best = 0;
        for (int32_t c = 0; c < n_C; ++c) {
            acc.mutable_data()[c] = scores[(size_t)c].accuracy;
            const fsk_svm_cv_score &x = scores[(size_t)c], &b = scores[(size_t)best];
            if (x.accuracy > b.accuracy || (x.accuracy == b.accuracy && x.C < b.C)) best = c;
        }
        py::list problems;
        for (const fsk_svm_cv_problem& q : probs) {
            py::dict d = pair_dict((int32_t)q.reserved[0], (int32_t)q.reserved[1], q.n_rows, q.iterations, (bool)q.converged, q.gap, q.objective, q.rho,
                                   q.n_sv, q.n_bsv);
            d["C"] = q.C; d["fold"] = q.fold;
            problems.append(d);
        }
        py::dict d;
        d["pred"] = pred; d["accuracy"] = acc; d["problems"] = problems; d["k"] = k;
        d["form"] = info.form == 1 ? "workgroup" : "two-launch"; d["launches"] = info.launches; d["ms"] = info.ms;
        d["fold"] = fold; d["best_C"] = scores[(size_t)best].C; d["kernel_type"] = kernel_type;
        if (weighted) d["class_weight"] = w; else d["class_weight"] = py::none();
        if (refit) {
            py::object cw = py::none();
            if (weighted) {  // (the very weights, keyed by class)
                py::dict by_label;
                py::array_t<int32_t> classes = py::module_::import("numpy").attr("unique")(labels).cast<py::array_t<int32_t>>();
                for (py::ssize_t c = 0; c < classes.shape(0); ++c) by_label[py::int_(classes.data()[c])] = w.data()[c];
                cw = by_label;
            }
            d["refit"] = fit_svm_multiclass(labels, scores[(size_t)best].C, eps, max_iter, kernel_type, cw, probability, calibration_folds, seed);
        }
        return d;
    }
    py::array_t<double> get_dual_coef_np() const {  // alpha_i y_i, as scikit-learn's dual_coef_ (dense, every training row)
        py::array_t<double> out((py::ssize_t)n_train_);
        if (svr_) {  // (alpha - alpha*)
            check(fsk_svr_get_model(h_, nullptr, out.mutable_data(), nullptr, nullptr));
            return out;
        }
        check(fsk_svm_get_model(h_, out.mutable_data(), nullptr, nullptr));
        if ((int64_t)labels_.size() != n_train_) throw std::runtime_error("no model: call fit_svm first");
        double* a = out.mutable_data();
        for (int64_t t = 0; t < n_train_; ++t) a[t] = labels_[(size_t)t] > 0 ? a[t] : -a[t];
        return out;
    }
    double get_intercept() const {  // -rho, as scikit-learn's intercept_
        double rho = 0;
        check(svr_ ? fsk_svr_get_model(h_, nullptr, nullptr, &rho, nullptr) : fsk_svm_get_model(h_, nullptr, &rho, nullptr));
        return -rho;
    }
    void decision_rows(const std::string& which, int64_t* r0, int64_t* r1) const {
        if (which == "test") { *r0 = n_train_; *r1 = n_train_ + n_test_; }
        else if (which == "train") { *r0 = 0; *r1 = n_train_; }
        else throw py::value_error("which must be 'test' or 'train'");
    }
    // sum_i alpha_i y_i K(r, i) - rho of the test (or train) rows: only cells with a train column are read, so the
    // test x test block is neither needed nor computed (skip_test_block=True / "lazy")
    // With the model of fit_svm_multiclass: [rows, P], the pairs (a, b), a < b, in lexicographic order of the classes — the
    // columns of scikit-learn's decision_function_shape="ovo".
    py::array_t<double> decision_function_np(const std::string& which) const {
        int64_t r0, r1;
        decision_rows(which, &r0, &r1);
        fsk_svm_multiclass_info mi;
        if (fsk_svm_multiclass_get_model(h_, nullptr, nullptr, nullptr, &mi) == FSK_OK) {
            py::array_t<double> dec({(py::ssize_t)(r1 - r0), (py::ssize_t)mi.n_pairs});
            check(fsk_svm_multiclass_decision(h_, r0, r1, dec.mutable_data(), nullptr));
            return dec;
        }
        py::array_t<double> out((py::ssize_t)(r1 - r0));
        check(fsk_svm_decision(h_, r0, r1, out.mutable_data()));
        return out;
    }
    // P(y = +1) of the test (or train) rows: the calibration's sigmoid of the decision values (fsk_svm_proba), a host array.
    // With the calibrated model of fit_svm_multiclass(probability=True): [rows, k], the coupled class probabilities of
    // fsk_svm_multiclass_proba, columns in the order of `classes`; uncalibrated it raises, naming the model.
    py::array_t<double> predict_proba_np(const std::string& which) const {
        int64_t r0, r1;
        decision_rows(which, &r0, &r1);
        fsk_svm_multiclass_info mi;
        if (fsk_svm_multiclass_get_model(h_, nullptr, nullptr, nullptr, &mi) == FSK_OK) {
            if (fsk_svm_multiclass_get_calibration(h_, nullptr, nullptr) != FSK_OK)
                throw std::runtime_error("predict_proba_np: the model is a multi-class C-SVC (fsk_svm_train_multiclass) without a calibration: "
                                         "fit_svm_multiclass(..., probability=True)");
            py::array_t<double> prob({(py::ssize_t)(r1 - r0), (py::ssize_t)mi.k});
            check(fsk_svm_multiclass_proba(h_, r0, r1, prob.mutable_data(), nullptr, nullptr));
            return prob;
        }
        py::array_t<double> out((py::ssize_t)(r1 - r0));
        check(fsk_svm_proba(h_, r0, r1, out.mutable_data()));
        return out;
    }
    // the same [rows, k] left on the device (fsk_svm_multiclass_proba_device), no copy; the multi-class model only
    py::capsule predict_proba_dlpack(const std::string& which) {
        int64_t r0, r1;
        decision_rows(which, &r0, &r1);
        if (r1 == r0) throw py::value_error("no rows");
        fsk_svm_multiclass_info mi;
        check(fsk_svm_multiclass_get_model(h_, nullptr, nullptr, nullptr, &mi));  // (RuntimeError before anything is allocated)
        check(fsk_svm_multiclass_get_calibration(h_, nullptr, nullptr));
        double* dev = nullptr;
        check(fsk_alloc_block_device(h_, r0, r1, 0, mi.k, &dev));  // the engine's allocator: (r1 - r0) x k doubles
        const int rc = fsk_svm_multiclass_proba_device(h_, r0, r1, dev, nullptr, nullptr);
        if (rc != FSK_OK) (void)fsk_free_device(h_, dev);
        check(rc);
        return dlpack_of(dev, 2, r1 - r0, mi.k);
    }
    py::capsule decision_function_dlpack(const std::string& which) {
        int64_t r0, r1;
        decision_rows(which, &r0, &r1);
        if (r1 == r0) throw py::value_error("no rows");
        double rho = 0;
        check(svr_ ? fsk_svr_get_model(h_, nullptr, nullptr, &rho, nullptr) : fsk_svm_get_model(h_, nullptr, &rho, nullptr));  // (RuntimeError before anything is allocated)
        double* dev = nullptr;
        check(fsk_alloc_block_device(h_, r0, r1, 0, 1, &dev));  // the engine's allocator: a column of r1 - r0 doubles
        const int rc = fsk_svm_decision_device(h_, r0, r1, dev);
        if (rc != FSK_OK) (void)fsk_free_device(h_, dev);
        check(rc);
        return dlpack_of(dev, 1, r1 - r0, 1);
    }
    void fit(double, double, double, const std::string&) const {
        PyErr_SetString(PyExc_NotImplementedError,
                        "fit(): the LIBSVM stage is outside the accelerated path; feed get_train_kernel() to scikit-learn "
                        "as the reference's own pipeline does (test/run_check.py:48-61)");
        throw py::error_already_set();
    }
    double score(const std::string&) const {
        PyErr_SetString(PyExc_NotImplementedError, "score(): see fit()");
        throw py::error_already_set();
    }
};

}  // namespace

PYBIND11_MODULE(_fastsk, m) {
    m.doc() = "MI355X-native gapped-k-mer kernel engine behind the FastSK Python surface";
    py::class_<FastSK>(m, "FastSK")
        // (two overloads: the signature as it was, wildcards its last keyword, by position or by name; and the same followed
        // by center_weights, keyword-only and without a default, so that a call that does not name it is the first's)
        .def(py::init([](int g, int m, int t, bool approx, double delta, int max_iters, bool skip_variance, int device,
                         const std::string& path, py::object seed, py::object skip_test_block, py::object devices,
                         const std::string& collective, int deadline_ms, py::object revcomp, py::object weights,
                         py::object max_mismatches, py::object wildcards) {
                 return new FastSK(g, m, t, approx, delta, max_iters, skip_variance, device, path, seed, skip_test_block, devices,
                                   collective, deadline_ms, revcomp, weights, max_mismatches, wildcards, py::none());
             }),
             py::arg("g"), py::arg("m"), py::arg("t") = -1, py::arg("approx") = false, py::arg("delta") = 0.025,
             py::arg("max_iters") = -1, py::arg("skip_variance") = false, py::arg("device") = 0,
             py::arg("path") = "auto", py::arg("seed") = py::none(), py::arg("skip_test_block") = false,
             py::arg("devices") = py::none(), py::arg("collective") = "auto", py::arg("deadline_ms") = 0,
             py::arg("revcomp") = py::none(), py::arg("weights") = py::none(), py::arg("max_mismatches") = py::none(),
             py::arg("wildcards") = py::none())
        .def(py::init<int, int, int, bool, double, int, bool, int, const std::string&, py::object, py::object, py::object,
                      const std::string&, int, py::object, py::object, py::object, py::object, py::object>(),
             py::arg("g"), py::arg("m"), py::arg("t") = -1, py::arg("approx") = false, py::arg("delta") = 0.025,
             py::arg("max_iters") = -1, py::arg("skip_variance") = false, py::arg("device") = 0,
             py::arg("path") = "auto", py::arg("seed") = py::none(), py::arg("skip_test_block") = false,
             py::arg("devices") = py::none(), py::arg("collective") = "auto", py::arg("deadline_ms") = 0,
             py::arg("revcomp") = py::none(), py::arg("weights") = py::none(), py::arg("max_mismatches") = py::none(),
             py::arg("wildcards") = py::none(), py::kw_only(), py::arg("center_weights"))
        .def("compute_kernel", &FastSK::compute_kernel, py::arg("Xtrain"), py::arg("Xtest"))
        .def("compute_kernel_flat", &FastSK::compute_kernel_flat, py::arg("tokens").noconvert(), py::arg("offsets").noconvert(),
             py::arg("n_train"))
        .def("compute_train", &FastSK::compute_train, py::arg("Xtrain"))
        .def("get_train_kernel", &FastSK::get_train_kernel)
        .def("get_test_kernel", &FastSK::get_test_kernel)
        .def("get_stdevs", &FastSK::get_stdevs)
        .def("save_kernel", &FastSK::save_kernel)
        .def("fit", &FastSK::fit, py::arg("C") = 1.0, py::arg("nu") = 0.5, py::arg("eps") = 0.001,
             py::arg("kernel_type") = "linear")
        .def("score", &FastSK::score, py::arg("metric") = "auc")
        // additive, non-breaking extras
        .def("get_train_kernel_np", &FastSK::get_train_kernel_np)
        .def("get_test_kernel_np", &FastSK::get_test_kernel_np)
        .def("get_block", &FastSK::get_block, py::arg("i0"), py::arg("i1"), py::arg("j0"), py::arg("j1"))
        .def("get_train_kernel_dlpack", &FastSK::get_train_kernel_dlpack)
        .def("get_test_kernel_dlpack", &FastSK::get_test_kernel_dlpack)
        .def("get_block_dlpack", &FastSK::get_block_dlpack, py::arg("i0"), py::arg("i1"), py::arg("j0"), py::arg("j1"))
        .def("get_counts_np", &FastSK::get_counts_np)
        .def("counts_digest", &FastSK::counts_digest, py::arg("row_begin") = 0, py::arg("row_end") = -1)
        .def("get_counts_block", &FastSK::get_counts_block, py::arg("i0"), py::arg("i1"), py::arg("j0"), py::arg("j1"))
        .def("get_counts_cells", &FastSK::get_counts_cells, py::arg("rows"), py::arg("cols"))
        .def("get_triangle_dlpack", &FastSK::get_triangle_dlpack)
        .def("set_combo_order", &FastSK::set_combo_order, py::arg("order"))
        .def("mismatch_info", &FastSK::mismatch_info)
        .def("fit_svm", &FastSK::fit_svm, py::arg("labels"), py::arg("C") = 1.0, py::arg("eps") = 1e-3, py::arg("max_iter") = -1,
             py::arg("kernel_type") = "fastsk", py::arg("class_weight") = py::none(), py::arg("probability") = false,
             py::arg("calibration_folds") = 5, py::arg("seed") = 0)
        .def("get_rows_kernel_block_np", &FastSK::get_rows_kernel_block_np, py::arg("i0"), py::arg("i1"), py::arg("j0"), py::arg("j1"),
             py::arg("raw") = false)
        .def("rows_kernel_info", &FastSK::rows_kernel_info)
        .def("cross_validate_svm", &FastSK::cross_validate_svm, py::arg("labels"), py::arg("Cs") = std::vector<double>{1.0},
             py::arg("folds") = 5, py::arg("eps") = 1e-3, py::arg("max_iter") = -1, py::arg("seed") = 0, py::arg("refit") = false,
             py::arg("kernel_type") = "fastsk", py::arg("class_weight") = py::none())
        .def("get_dual_coef_np", &FastSK::get_dual_coef_np)
        .def("get_intercept", &FastSK::get_intercept)
        .def("decision_function_np", &FastSK::decision_function_np, py::arg("which") = "test")
        .def("decision_function_dlpack", &FastSK::decision_function_dlpack, py::arg("which") = "test")
        .def("predict_proba_np", &FastSK::predict_proba_np, py::arg("which") = "test")
        .def("fit_svr", &FastSK::fit_svr, py::arg("targets"), py::arg("C") = 1.0, py::arg("epsilon") = 0.1, py::arg("eps") = 1e-3,
             py::arg("max_iter") = -1, py::arg("kernel_type") = "fastsk")
        .def("cross_validate_svr", &FastSK::cross_validate_svr, py::arg("targets"), py::arg("Cs") = std::vector<double>{1.0},
             py::arg("epsilons") = std::vector<double>{0.1}, py::arg("folds") = 5, py::arg("seed") = 0, py::arg("eps") = 1e-3,
             py::arg("max_iter") = -1, py::arg("kernel_type") = "fastsk", py::arg("refit") = false)
        .def("predict_np", &FastSK::decision_function_np, py::arg("which") = "test")
        .def("predict_dlpack", &FastSK::decision_function_dlpack, py::arg("which") = "test")
        .def("fit_svm_multiclass", &FastSK::fit_svm_multiclass, py::arg("labels"), py::arg("C") = 1.0, py::arg("eps") = 1e-3,
             py::arg("max_iter") = -1, py::arg("kernel_type") = "fastsk", py::arg("class_weight") = py::none(),
             py::arg("probability") = false, py::arg("calibration_folds") = 5, py::arg("seed") = 0)
        .def("predict_class_np", &FastSK::predict_class_np, py::arg("which") = "test", py::arg("rule") = "vote")
        .def("predict_proba_dlpack", &FastSK::predict_proba_dlpack, py::arg("which") = "test")
        .def("cross_validate_svm_multiclass", &FastSK::cross_validate_svm_multiclass, py::arg("labels"),
             py::arg("Cs") = std::vector<double>{1.0}, py::arg("folds") = 5, py::arg("eps") = 1e-3, py::arg("max_iter") = -1,
             py::arg("seed") = 0, py::arg("refit") = false, py::arg("kernel_type") = "fastsk", py::arg("class_weight") = py::none(),
             py::arg("probability") = false, py::arg("calibration_folds") = 5)
        .def("stats", &FastSK::stats);
    // the level coefficients a_0..a_d of mismatch weights c_0..c_m at window length g (fsk_mismatch_levels; host only)
    m.def("mismatch_levels", [](int g, std::vector<uint64_t> weights) {
        std::vector<int64_t> a(weights.size() + 1);
        int32_t n = 0;
        if (fsk_mismatch_levels(g, weights.data(), (int32_t)weights.size(), a.data(), &n) != FSK_OK) throw py::value_error(fsk_last_error(nullptr));
        a.resize((size_t)n);
        return a;
    }, py::arg("g"), py::arg("weights"));
    m.attr("__version__") = "dev";
    m.attr("abi_version") = fsk_abi_version();
}
