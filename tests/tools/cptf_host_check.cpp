// cptf_host_check.cpp -- a stand-alone program over the host side of CPTF (carskit_amd/csrc/cptf_host.hpp: the tensor build, the fold
// split, getKeys), on random rating matrices and the edge cases, for a run under AddressSanitizer and UndefinedBehaviorSanitizer.  No
// device:
//
//   hipcc --offload-host-only -x hip -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Icarskit_amd/csrc tests/tools/cptf_host_check.cpp -o cptf_host_check && ./cptf_host_check
#include <algorithm>
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "cptf_host.hpp"

using namespace cmi;

static int failures = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__);     \
            ++failures;                                             \
        }                                                           \
    } while (0)

struct Problem {
    std::vector<int32_t> pair, ctx, pair_user, pair_item, ctx_ptr, ctx_conds, cond_dim, test_pair;
    std::vector<double> rate;
    CptfTensorIn in(bool indexof) const {
        CptfTensorIn a;
        a.n_cells = (int64_t)pair.size(), a.pair = pair.data(), a.ctx = ctx.data(), a.rate = rate.data();
        a.n_pairs = (int32_t)pair_user.size(), a.pair_user = pair_user.data(), a.pair_item = pair_item.data();
        a.n_ctx = (int32_t)ctx_ptr.size() - 1, a.ctx_ptr = ctx_ptr.data(), a.ctx_conds = ctx_conds.data();
        a.n_conds = (int32_t)cond_dim.size(), a.cond_dim = cond_dim.data();
        a.n_test = (int64_t)test_pair.size(), a.test_pair = test_pair.data(), a.keys_indexof = indexof;
        return a;
    }
};

// every user and item occurs (ids dense), every condition of every dimension occurs in some rated context
static Problem random_problem(std::mt19937 &rng, int nu, int ni, const std::vector<int> &per_dim, int n_ctx, int extra, int n_test) {
    Problem p;
    std::vector<int> first;
    for (size_t d = 0; d < per_dim.size(); ++d) {
        first.push_back((int)p.cond_dim.size());
        for (int x = 0; x < per_dim[d]; ++x) p.cond_dim.push_back((int32_t)d);
    }
    p.ctx_ptr.push_back(0);
    for (int c = 0; c < n_ctx; ++c) {
        for (size_t d = 0; d < per_dim.size(); ++d) p.ctx_conds.push_back(first[d] + (int)(rng() % (unsigned)per_dim[d]));
        p.ctx_ptr.push_back((int32_t)p.ctx_conds.size());
    }
    std::set<std::pair<int, int>> pairs;
    for (int u = 0; u < nu; ++u) pairs.insert({u, (int)(rng() % (unsigned)ni)});
    for (int i = 0; i < ni; ++i) pairs.insert({(int)(rng() % (unsigned)nu), i});
    for (int x = 0; x < extra; ++x) pairs.insert({(int)(rng() % (unsigned)nu), (int)(rng() % (unsigned)ni)});
    for (auto &pr : pairs) p.pair_user.push_back(pr.first), p.pair_item.push_back(pr.second);
    std::set<std::pair<int, int>> cells;
    for (int q = 0; q < (int)pairs.size(); ++q) cells.insert({q, (int)(rng() % (unsigned)n_ctx)});
    for (int x = 0; x < 2 * extra; ++x) cells.insert({(int)(rng() % (unsigned)pairs.size()), (int)(rng() % (unsigned)n_ctx)});
    for (auto &c : cells) p.pair.push_back(c.first), p.ctx.push_back(c.second), p.rate.push_back(1.0 + (double)(rng() % 5));
    std::set<int> test;
    while ((int)test.size() < std::min<int>(n_test, (int)p.pair.size())) test.insert((int)(rng() % (unsigned)p.pair.size()));
    for (int t : test) p.test_pair.push_back(p.pair[(size_t)t]);
    return p;
}

static void check(const Problem &p, bool indexof) {
    CptfTensorOut o;
    std::string err;
    const int rc = cptf_tensor_build(p.in(indexof), o, err);
    if (rc != CPTF_BUILD_OK) {   // only contexts that no cell rates can miss a condition
        CHECK(rc == CPTF_BUILD_INVALID && err.find("getKeys gives -1") != std::string::npos);
        return;
    }
    const size_t nd = o.dims.size(), n = p.pair.size();
    CHECK(o.keys.size() == n * nd && o.vals.size() == n);
    for (size_t t = 0; t < n; ++t)
        for (size_t d = 0; d < nd; ++d) CHECK(o.keys[t * nd + d] >= 0 && o.keys[t * nd + d] < o.dims[d]);   // (ids are dense here)
    for (size_t d = 2; d < nd; ++d) CHECK((int32_t)o.dim_lists[d - 2].size() == o.dims[d]);
    // the fold: train and test partition the rate tensor by pair; the test tensor holds every distinct key tuple of the test pairs once
    std::set<int> test_pairs(p.test_pair.begin(), p.test_pair.end());
    size_t n_train = 0;
    std::set<std::vector<int32_t>> test_keys;
    for (size_t t = 0; t < n; ++t) {
        std::vector<int32_t> ks(o.keys.begin() + (long)(t * nd), o.keys.begin() + (long)((t + 1) * nd));
        if (test_pairs.count(p.pair[t])) test_keys.insert(ks);
        else {
            CHECK(n_train < o.train_vals.size() && std::equal(ks.begin(), ks.end(), o.train_keys.begin() + (long)(n_train * nd)) &&
                  o.train_vals[n_train] == p.rate[t]);
            ++n_train;
        }
    }
    CHECK(n_train == o.train_vals.size() && o.train_keys.size() == n_train * nd);
    CHECK(o.test_vals.size() == test_keys.size() && o.test_keys.size() == test_keys.size() * nd);
    std::set<std::vector<int32_t>> got;
    for (size_t t = 0; t < o.test_vals.size(); ++t)
        got.insert(std::vector<int32_t>(o.test_keys.begin() + (long)(t * nd), o.test_keys.begin() + (long)((t + 1) * nd)));
    CHECK(got == test_keys);
    if (indexof) {   // the corrected form: training keys of a cell are its context's ranking keys, and no two cells collapse
        for (size_t t = 0; t < n; ++t)
            for (size_t d = 2; d < nd; ++d) CHECK(o.keys[t * nd + d] == o.ctx_keys[(size_t)p.ctx[t] * (nd - 2) + (d - 2)]);
    }
}

int main() {
    std::mt19937 rng(20271021);
    for (int round = 0; round < 200; ++round) {
        const int nu = 1 + (int)(rng() % 9), ni = 1 + (int)(rng() % 9);
        std::vector<int> per_dim(1 + rng() % 8);
        for (int &x : per_dim) x = 1 + (int)(rng() % 4);
        const Problem p = random_problem(rng, nu, ni, per_dim, 1 + (int)(rng() % 12), (int)(rng() % 60), (int)(rng() % 10));
        check(p, false);
        check(p, true);
    }
    {   // one user with 300 positions: the HashSet of positions grows past 64 slots
        const Problem p = random_problem(rng, 1, 300, {3}, 3, 0, 40);
        check(p, false);
        check(p, true);
    }
    {   // refusals
        Problem p = random_problem(rng, 3, 3, {2, 2}, 4, 5, 2);
        CptfTensorOut o;
        std::string err;
        Problem q = p;
        q.cond_dim.assign(q.cond_dim.size(), 0);   // every context now holds two conditions of dimension 0
        CHECK(cptf_tensor_build(q.in(false), o, err) == CPTF_BUILD_INVALID);
        q = p;
        q.pair_user[0] = 7;                        // an id not below the number of distinct users builds, as in the reference
        CHECK(cptf_tensor_build(q.in(false), o, err) == CPTF_BUILD_OK && o.dims[0] <= 4);
        q.test_pair.assign(1, 0);
        CHECK(cptf_tensor_build(q.in(false), o, err) == CPTF_BUILD_OK && !o.test_vals.empty() && o.test_keys[0] == 7);
        q.pair_user[0] = 2147483647, q.pair_item[1] = 2147483646;   // the largest ids: nothing is sized by an id
        CHECK(cptf_tensor_build(q.in(false), o, err) == CPTF_BUILD_OK && !o.test_vals.empty() && o.test_keys[0] == 2147483647);
        q = p;
        q.pair[0] = (int32_t)q.pair_user.size();
        CHECK(cptf_tensor_build(q.in(false), o, err) == CPTF_BUILD_INVALID);
        q = p;
        q.cond_dim.clear(), q.ctx_conds.clear(), q.ctx_ptr.assign(q.ctx_ptr.size(), 0);   // no context dimension
        CHECK(cptf_tensor_build(q.in(false), o, err) == CPTF_BUILD_UNSUPPORTED);
        Problem e;                                 // nothing at all
        e.ctx_ptr.push_back(0);
        CHECK(cptf_tensor_build(e.in(false), o, err) == CPTF_BUILD_UNSUPPORTED);
    }
    if (failures) {
        std::printf("%d cptf host checks FAILED\n", failures);
        return 1;
    }
    std::printf("cptf host checks passed\n");
    return 0;
}
