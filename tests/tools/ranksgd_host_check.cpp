// ranksgd_host_check.cpp -- a stand-alone program over the host side of RankSGD (ranksgd_host.hpp): the item list, the tries and the
// walk that assigns them, on random matrices and the edge cases, for a run under AddressSanitizer and UndefinedBehaviorSanitizer.
// No device: the header's shared functions are compiled for the host only.
//
//   hipcc --offload-host-only -x hip -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Icarskit_amd/csrc tests/tools/ranksgd_host_check.cpp -o ranksgd_host_check && ./ranksgd_host_check
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "ranksgd_host.hpp"

using namespace cmi;

static int failures = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__);     \
            ++failures;                                             \
        }                                                           \
    } while (0)

struct Csr {
    std::vector<int32_t> ptr, idx;
};

static Csr random_matrix(std::mt19937 &rng, int nu, int ni, int max_per_user) {
    Csr m;
    m.ptr.assign((size_t)nu + 1, 0);
    for (int u = 0; u < nu; ++u) {
        std::set<int> row;
        const int cnt = (int)(rng() % (unsigned)(std::min(ni, max_per_user) + 1));
        while ((int)row.size() < cnt) row.insert((int)(rng() % (unsigned)ni));
        for (int j : row) m.idx.push_back(j);
        m.ptr[(size_t)u + 1] = (int32_t)m.idx.size();
    }
    return m;
}

static void check(const Csr &m, int nu, int ni, int64_t num_rates, uint64_t state) {
    std::vector<int32_t> col((size_t)ni, 0);
    for (int32_t j : m.idx) ++col[(size_t)j];
    const RanksgdTable t = ranksgd_item_table(ni, col.data(), num_rates < 0 ? (int64_t)m.idx.size() : num_rates);
    const int32_t n = (int32_t)t.item.size();
    std::set<int32_t> seen(t.item.begin(), t.item.end());
    CHECK((int32_t)seen.size() == n && t.cum.size() == t.item.size() && t.prob.size() == t.item.size());
    for (int32_t j = 0; j < ni; ++j) CHECK((col[(size_t)j] > 0) == (seen.count(j) == 1));
    for (int32_t x = 1; x < n; ++x) CHECK(t.prob[(size_t)x - 1] <= t.prob[(size_t)x] && t.cum[(size_t)x - 1] <= t.cum[(size_t)x]);
    if (n == 0) return;
    CHECK(ranksgd_reservation(nu, ni, m.ptr.data(), m.idx.data(), t) >= (double)m.idx.size());
    if (t.tree || ranksgd_endless_user(nu, m.ptr.data(), m.idx.data(), t) >= 0) return;
    // the walk over tries computed ahead equals the walk that computes them as it goes; both end
    const JavaLcgJump jump = java_lcg_jump_table();
    const int64_t ahead = (int64_t)m.idx.size() + 7;
    std::vector<int32_t> tries((size_t)ahead);
    for (int64_t q = 0; q < ahead; ++q) {
        tries[(size_t)q] = ranksgd_try(java_lcg_jump(jump, state, 2 * (uint64_t)q), t.item.data(), t.cum.data(), n);
        CHECK(tries[(size_t)q] >= -1 && tries[(size_t)q] < ni);
    }
    auto host = [&](int64_t q) { return ranksgd_try(java_lcg_jump(jump, state, 2 * (uint64_t)q), t.item.data(), t.cum.data(), n); };
    std::vector<int32_t> j1(m.idx.size() + 1), j2(m.idx.size() + 1);
    int64_t used1 = 0, used2 = 0, bad1 = 0, bad2 = 0;
    const int64_t cap = (int64_t)1 << 22;
    const int rc1 = ranksgd_assign(nu, m.ptr.data(), m.idx.data(), [&](int64_t q) { return q < ahead ? tries[(size_t)q] : host(q); }, cap,
                                   j1.data(), &used1, &bad1);
    const int rc2 = ranksgd_assign(nu, m.ptr.data(), m.idx.data(), host, cap, j2.data(), &used2, &bad2);
    CHECK(rc1 == rc2 && used1 == used2 && bad1 == bad2);
    if (rc1 == RANKSGD_OK) {
        CHECK(j1 == j2 && used1 >= (int64_t)m.idx.size());
        size_t c = 0;
        for (int u = 0; u < nu; ++u)
            for (int32_t q = m.ptr[(size_t)u]; q < m.ptr[(size_t)u + 1]; ++q, ++c)
                CHECK(!bpr_contains(m.idx.data() + m.ptr[(size_t)u], m.ptr[(size_t)u + 1] - m.ptr[(size_t)u], j1[c]));
    }
    // a walk that runs out of tries says so and writes no cell past the one it stopped at
    int64_t used3 = 0, bad3 = 0;
    std::vector<int32_t> j3(m.idx.size() + 1, -7);
    const int rc3 = ranksgd_assign(nu, m.ptr.data(), m.idx.data(), host, (int64_t)m.idx.size() / 2, j3.data(), &used3, &bad3);
    if (!m.idx.empty() && rc3 == RANKSGD_OUT_OF_TRIES) {
        CHECK(used3 == (int64_t)m.idx.size() / 2 && bad3 <= used3);
        for (size_t c = (size_t)bad3; c < j3.size(); ++c) CHECK(j3[c] == -7);
    }
}

int main() {
    std::mt19937 rng(20270312);
    for (int t = 0; t < 600; ++t) {
        const int nu = 1 + (int)(rng() % 40), ni = 1 + (int)(rng() % 90);
        const Csr m = random_matrix(rng, nu, ni, t % 3 == 0 ? 2 : 11);
        check(m, nu, ni, t % 2 ? -1 : 0, (uint64_t)rng() << 16 | (rng() & 0xffff));
    }
    {   // the empty matrix; ids that collide in a 16-slot table; ids past 65 535; a list large enough to grow the table
        Csr e;
        e.ptr.assign(4, 0);
        check(e, 3, 5, -1, 1);
        Csr c{{0, 4, 7, 9}, {1, 2, 17, 33, 17, 18, 34, 3, 19}};
        check(c, 3, 40, -1, 2), check(c, 3, 40, 0, 2);
        Csr big{{0, 4, 9}, {5, 16, 65536, 69999, 3, 131, 40000, 65552, 66000}};
        check(big, 2, 70000, -1, 3), check(big, 2, 70000, 0, 3);
        const Csr wide = random_matrix(rng, 300, 5000, 40);
        check(wide, 300, 5000, -1, 4);
    }
    {   // a list whose last sum is below 1: tries of -1
        const int32_t item[3] = {4, 1, 2};
        const double cum[3] = {0.125, 0.25, 0.5};
        const JavaLcgJump jump = java_lcg_jump_table();
        int none = 0;
        for (int q = 0; q < 4000; ++q) none += ranksgd_try(java_lcg_jump(jump, 99, 2 * (uint64_t)q), item, cum, 3) < 0;
        CHECK(none > 1700 && none < 2300);
        CHECK(ranksgd_reachable(cum, 0) && ranksgd_reachable(cum, 2));
        const double flat[3] = {INFINITY, INFINITY, INFINITY};
        CHECK(ranksgd_reachable(flat, 0) && !ranksgd_reachable(flat, 1) && !ranksgd_reachable(flat, 2));
    }
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("ranksgd host checks passed\n");
    return failures ? 1 : 0;
}
