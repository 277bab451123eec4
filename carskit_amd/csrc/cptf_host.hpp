// cptf_host.hpp -- the host side of CPTF without a device: DataDAO.toSparseTensor (DataDAO.java:423-481), the fold split of
// TensorRecommender's constructor (TensorRecommender.java:62-84) over librec's SparseTensor, and getKeys (:189-205).  No HIP: the
// stand-alone check tests/tools/cptf_host_check.cpp includes this file alone.  What SparseTensor does was found by executing the jar
// (tests/golden/reference_cptf.json.gz, `tensors`):
//   * getIndices(u, i) walks the positions of user u in the java.util.HashSet that guava's HashMultimap keeps per key -- new HashSet(3),
//     4 slots (java_hash.hpp) -- and keeps those of item i;
//   * set() on keys already present overwrites the value in place, so contexts of a pair that share keys become one test entry that
//     holds the value set last;
//   * remove() deletes one matching entry and keeps the order of the rest; every index of a test pair is removed, so the train tensor is
//     the rate tensor without the test pairs' entries -- all their contexts -- in order.
#pragma once
#include <cstdint>
#include <cstdio>
#include <map>
#include <unordered_map>
#include <unordered_set>
#include <string>
#include <vector>

#include "java_hash.hpp"

namespace cmi {

constexpr int CPTF_BUILD_OK = 0, CPTF_BUILD_INVALID = 1, CPTF_BUILD_UNSUPPORTED = 2;
constexpr int CPTF_BUILD_MAX_DIMS = 10;

struct CptfTensorIn {
    int64_t n_cells = 0;                      // rateMatrix in its iteration order: rows (user-item pairs), then columns (contexts)
    const int32_t *pair = nullptr, *ctx = nullptr;
    const double *rate = nullptr;
    int32_t n_pairs = 0;
    const int32_t *pair_user = nullptr, *pair_item = nullptr;
    int32_t n_ctx = 0;                        // context c holds the conditions ctx_conds[ctx_ptr[c] .. ctx_ptr[c + 1]) in list order
    const int32_t *ctx_ptr = nullptr, *ctx_conds = nullptr;
    int32_t n_conds = 0;
    const int32_t *cond_dim = nullptr;        // condition -> context dimension, the dimensions numbered 0 .. D - 1
    int64_t n_test = 0;                       // testMatrix in its iteration order: the pair of every cell
    const int32_t *test_pair = nullptr;
    bool keys_indexof = false;                // false: DataDAO.java:461 as it stands (a listed condition gets the list's last index)
};

struct CptfTensorOut {
    std::vector<int32_t> dims;                          // 2 + D
    std::vector<std::vector<int32_t>> dim_lists;        // per context dimension: its conditions in list order
    std::vector<int32_t> keys, train_keys, test_keys;   // entries x dims.size(), each tensor in its iterator order
    std::vector<double> vals, train_vals, test_vals;
    std::vector<int32_t> ctx_keys;                      // n_ctx x D: getKeys' keys of every context
};

inline int cptf_build_fail(std::string &err, int code, const char *fmt, long long a = 0, long long b = 0, long long c = 0) {
    char buf[320];
    std::snprintf(buf, sizeof buf, fmt, a, b, c);
    err = buf;
    return code;
}

inline int cptf_tensor_build(const CptfTensorIn &in, CptfTensorOut &out, std::string &err) {
    out = CptfTensorOut();
    if (in.n_cells < 0 || in.n_pairs < 0 || in.n_ctx < 0 || in.n_conds < 0 || in.n_test < 0 || in.n_cells >= ((int64_t)1 << 31) ||
        (in.n_cells > 0 && (!in.pair || !in.ctx || !in.rate)) || (in.n_pairs > 0 && (!in.pair_user || !in.pair_item)) ||
        (in.n_ctx > 0 && (!in.ctx_ptr || (in.ctx_ptr[in.n_ctx] > 0 && !in.ctx_conds))) || (in.n_conds > 0 && !in.cond_dim) ||
        (in.n_test > 0 && !in.test_pair))
        return cptf_build_fail(err, CPTF_BUILD_INVALID, "invalid argument");
    int D = 0;
    for (int32_t c = 0; c < in.n_conds; ++c) {
        if (in.cond_dim[c] < 0 || in.cond_dim[c] >= CPTF_BUILD_MAX_DIMS)
            return cptf_build_fail(err, CPTF_BUILD_INVALID, "condition %lld: dimension %lld out of range", c, in.cond_dim[c]);
        if (in.cond_dim[c] + 1 > D) D = in.cond_dim[c] + 1;
    }
    if (D < 1) return cptf_build_fail(err, CPTF_BUILD_UNSUPPORTED, "no context dimension: librec's SparseTensor refuses fewer than 3 dimensions");
    if (2 + D > CPTF_BUILD_MAX_DIMS) return cptf_build_fail(err, CPTF_BUILD_UNSUPPORTED, "%lld tensor dimensions, more than 10", 2 + D);
    // every context: one condition of every dimension (ndLists of one length, DataDAO.java:470)
    for (int32_t c = 0; c < in.n_ctx; ++c) {
        if (in.ctx_ptr[c] < 0 || in.ctx_ptr[c + 1] < in.ctx_ptr[c]) return cptf_build_fail(err, CPTF_BUILD_INVALID, "context %lld: list bounds", c);
        unsigned seen = 0;
        for (int32_t q = in.ctx_ptr[c]; q < in.ctx_ptr[c + 1]; ++q) {
            const int32_t cond = in.ctx_conds[q];
            if (cond < 0 || cond >= in.n_conds) return cptf_build_fail(err, CPTF_BUILD_INVALID, "context %lld: condition %lld out of range", c, cond);
            if (seen & (1u << in.cond_dim[cond]))
                return cptf_build_fail(err, CPTF_BUILD_INVALID, "context %lld holds two conditions of dimension %lld", c, in.cond_dim[cond]);
            seen |= 1u << in.cond_dim[cond];
        }
        if (seen != (1u << D) - 1) return cptf_build_fail(err, CPTF_BUILD_INVALID, "context %lld lacks a condition of some dimension", c);
    }
    for (int64_t t = 0; t < in.n_cells; ++t)
        if (in.pair[t] < 0 || in.pair[t] >= in.n_pairs || in.ctx[t] < 0 || in.ctx[t] >= in.n_ctx)
            return cptf_build_fail(err, CPTF_BUILD_INVALID, "cell %lld: pair or context out of range", t);
    for (int64_t t = 0; t < in.n_test; ++t)
        if (in.test_pair[t] < 0 || in.test_pair[t] >= in.n_pairs) return cptf_build_fail(err, CPTF_BUILD_INVALID, "test cell %lld: pair out of range", t);
    for (int32_t p = 0; p < in.n_pairs; ++p)
        if (in.pair_user[p] < 0 || in.pair_item[p] < 0) return cptf_build_fail(err, CPTF_BUILD_INVALID, "pair %lld: negative id", p);

    // DataDAO.java:437-473
    const int nd = 2 + D;
    out.dim_lists.assign((size_t)D, {});
    std::vector<uint8_t> dim_started((size_t)D, 0);
    std::vector<std::unordered_set<int32_t>> seen_key((size_t)nd); // (a set, not a table sized by the largest id: ids are the caller's)
    auto note = [&](int d, int32_t key) { seen_key[(size_t)d].insert(key); };
    out.keys.resize((size_t)in.n_cells * (size_t)nd);
    out.vals.assign(in.rate, in.rate + in.n_cells);
    for (int64_t t = 0; t < in.n_cells; ++t) {
        int32_t *ks = &out.keys[(size_t)t * (size_t)nd];
        ks[0] = in.pair_user[in.pair[t]], ks[1] = in.pair_item[in.pair[t]];
        for (int32_t q = in.ctx_ptr[in.ctx[t]]; q < in.ctx_ptr[in.ctx[t] + 1]; ++q) {
            const int32_t cond = in.ctx_conds[q], dim = in.cond_dim[cond];
            std::vector<int32_t> &list = out.dim_lists[(size_t)dim];
            int32_t index = -1;
            if (dim_started[(size_t)dim]) {                                // :456-462
                for (size_t x = 0; x < list.size() && index < 0; ++x)
                    if (list[x] == cond) index = (int32_t)x;
                const bool found = index >= 0;
                if (!found) list.push_back(cond);
                if (!found || !in.keys_indexof) index = (int32_t)list.size() - 1;   // :461, not under the `if`
            } else {                                                       // :463-469
                list.push_back(cond), dim_started[(size_t)dim] = 1, index = 0;
            }
            ks[2 + dim] = index;
        }
        for (int d = 0; d < nd; ++d) note(d, ks[d]);
    }
    for (int d = 0; d < nd; ++d) out.dims.push_back((int32_t)seen_key[(size_t)d].size());   // :474-476: the sizes of the key SETS
    // (the reference sizes M[d] by these counts and indexes it with the key itself: a user or item id that is not below the number of
    // distinct ids builds here as it does there, and is out of range for the model -- cmi_cptf_set_entries refuses it)

    // TensorRecommender.java:189-205: the k-th condition of a context is looked up in dimension k's list
    out.ctx_keys.resize((size_t)in.n_ctx * (size_t)D);
    for (int32_t c = 0; c < in.n_ctx; ++c)
        for (int k = 0; k < D; ++k) {
            const int32_t cond = in.ctx_conds[in.ctx_ptr[c] + k];
            const std::vector<int32_t> &list = out.dim_lists[(size_t)k];
            int32_t index = -1;
            for (size_t x = 0; x < list.size() && index < 0; ++x)
                if (list[x] == cond) index = (int32_t)x;
            if (index < 0)
                return cptf_build_fail(err, CPTF_BUILD_INVALID,
                                       "context %lld: getKeys gives -1 for dimension %lld, condition %lld (TensorRecommender.java:199-201 logs "
                                       "and then indexes row -1)",
                                       c, k, cond);
            out.ctx_keys[(size_t)c * (size_t)D + (size_t)k] = index;
        }

    // TensorRecommender.java:66-83
    std::vector<uint8_t> is_test((size_t)in.n_pairs, 0);
    for (int64_t t = 0; t < in.n_test; ++t) is_test[(size_t)in.test_pair[t]] = 1;
    std::unordered_map<int32_t, std::vector<int32_t>> positions, ordered;   // of a user, ascending / HashSet order
    for (int64_t t = 0; t < in.n_cells; ++t) positions[out.keys[(size_t)t * (size_t)nd]].push_back((int32_t)t);
    for (int64_t t = 0; t < in.n_cells; ++t)
        if (!is_test[(size_t)in.pair[t]]) {
            out.train_keys.insert(out.train_keys.end(), &out.keys[(size_t)t * (size_t)nd], &out.keys[(size_t)t * (size_t)nd] + nd);
            out.train_vals.push_back(in.rate[t]);
        }
    std::map<std::vector<int32_t>, size_t> test_at;                        // keys -> entry of the test tensor
    for (int64_t t = 0; t < in.n_test; ++t) {
        const int32_t u = in.pair_user[in.test_pair[t]], i = in.pair_item[in.test_pair[t]];
        if (!positions.count(u)) continue;                                     // a pair without a cell: getIndices finds nothing
        if (!ordered.count(u)) {
            const std::vector<int32_t> &pos = positions[u];
            std::vector<int32_t> &ord = ordered[u];
            JavaHashTable table(4);                                        // guava's HashMultimap: new HashSet(3)
            auto hash_at = [&](size_t s) { return (uint32_t)pos[s]; };
            table.fill(hash_at, pos.size());
            if (table.tree)
                return cptf_build_fail(err, CPTF_BUILD_UNSUPPORTED,
                                       "user %lld: its positions would treeify a java.util.HashSet bin, whose iteration order is not modelled", u);
            for (size_t s : table.order(hash_at, pos.size())) ord.push_back(pos[s]);
        }
        for (int32_t p : ordered[u]) {
            if (out.keys[(size_t)p * (size_t)nd + 1] != i) continue;
            std::vector<int32_t> ks(&out.keys[(size_t)p * (size_t)nd], &out.keys[(size_t)p * (size_t)nd] + nd);
            auto it = test_at.find(ks);
            if (it != test_at.end()) {
                out.test_vals[it->second] = in.rate[p];                    // set() on keys already present
            } else {
                test_at.emplace(ks, out.test_vals.size());
                out.test_keys.insert(out.test_keys.end(), ks.begin(), ks.end());
                out.test_vals.push_back(in.rate[p]);
            }
        }
    }
    return CPTF_BUILD_OK;
}

} // namespace cmi
