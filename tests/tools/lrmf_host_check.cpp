// lrmf_host_check.cpp -- a stand-alone program over the host side of LRMF: the unit level builder (level_schedule.cpp) and what
// cmi_lrmf_set_ratings prepares (lrmf_host.hpp: userExp, A, the launch list), on random matrices and the edge cases, for a run under
// AddressSanitizer and UndefinedBehaviorSanitizer.  No HIP, no device:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Icarskit_amd/csrc
//       tests/tools/lrmf_host_check.cpp carskit_amd/csrc/level_schedule.cpp -o lrmf_host_check && ./lrmf_host_check
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "lrmf_host.hpp"

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
    std::vector<double> val;
};

static Csr random_matrix(std::mt19937 &rng, int nu, int ni, int max_per_user) {
    Csr m;
    m.ptr.assign((size_t)nu + 1, 0);
    for (int u = 0; u < nu; ++u) {
        std::set<int> row;
        const int cnt = (int)(rng() % (unsigned)(std::min(ni, max_per_user) + 1));
        while ((int)row.size() < cnt) row.insert((int)(rng() % (unsigned)ni));
        for (int j : row) m.idx.push_back(j), m.val.push_back((double)(rng() % 4)); // a quarter of the cells are stored zeros
        m.ptr[(size_t)u + 1] = (int32_t)m.idx.size();
    }
    return m;
}

static void check(const Csr &m, int nu, int ni, int lds_rows) {
    LrmfPlan p;
    lrmf_prepare(nu, ni, m.ptr.data(), m.idx.data(), m.val.data(), lds_rows, p);
    const size_t n = m.idx.size();
    CHECK(p.A.size() == n && p.nz.size() == n && p.user_exp.size() == (size_t)nu);
    CHECK(p.level_ptr.size() == (size_t)p.n_levels + 1);
    std::vector<int32_t> level_of;
    std::vector<int32_t> order, level_ptr;
    int64_t chain = 0;
    const int32_t nl = build_unit_levels(nu, ni, m.ptr.data(), m.idx.data(), order, level_ptr, &level_of, &chain);
    CHECK(nl == p.n_levels && order == p.order && level_ptr == p.level_ptr && chain == p.max_chain && nl >= chain);
    // every level row-disjoint, and the launches cover the order once, in sequence
    for (int32_t l = 0; l < nl; ++l) {
        std::set<int> seen;
        for (int32_t x = level_ptr[(size_t)l]; x < level_ptr[(size_t)l + 1]; ++x) {
            const int32_t u = order[(size_t)x];
            CHECK(level_of[(size_t)u] == l + 1);
            for (int32_t c = m.ptr[(size_t)u]; c < m.ptr[(size_t)u + 1]; ++c) CHECK(seen.insert(m.idx[(size_t)c]).second);
        }
    }
    int32_t at = 0;
    int64_t global_units = 0;
    for (const LrmfLaunch &l : p.launches) {
        CHECK(l.x0 == at && l.x1 > l.x0 && l.rows <= lds_rows);
        at = l.x1;
        for (int32_t x = l.x0; x < l.x1; ++x) {
            const int32_t u = order[(size_t)x], cnt = m.ptr[(size_t)u + 1] - m.ptr[(size_t)u];
            CHECK(cnt > lds_rows || cnt <= l.rows);
            global_units += cnt > lds_rows;
            if (l.run) CHECK(level_ptr[(size_t)level_of[(size_t)u]] - level_ptr[(size_t)level_of[(size_t)u] - 1] == 1);
        }
        if (!l.run) CHECK(level_of[(size_t)order[(size_t)l.x0]] == level_of[(size_t)order[(size_t)l.x1 - 1]] && l.x1 - l.x0 > 1);
        CHECK(lrmf_lds_bytes(16, l.rows) <= (size_t)LRMF_LDS_BYTES || l.rows > lrmf_lds_rows(16));
    }
    CHECK(at == (int32_t)order.size() && global_units == p.global_units);
    CHECK((int64_t)p.launches.size() == p.alone + p.runs);
    for (int u = 0; u < nu; ++u) {
        double s = 0.0;
        for (int32_t c = m.ptr[(size_t)u]; c < m.ptr[(size_t)u + 1]; ++c) s += fdlibm_exp(m.val[(size_t)c]);
        CHECK(s == p.user_exp[(size_t)u]);
        for (int32_t c = m.ptr[(size_t)u]; c < m.ptr[(size_t)u + 1]; ++c) CHECK(p.A[(size_t)c] > 0.0 && p.A[(size_t)c] <= 1.0);
    }
}

int main() {
    std::mt19937 rng(20270401);
    for (int t = 0; t < 400; ++t) {
        const int nu = 1 + (int)(rng() % 60), ni = 1 + (int)(rng() % 40);
        const Csr m = random_matrix(rng, nu, ni, t % 3 == 0 ? 2 : 9);
        check(m, nu, ni, t % 4 == 0 ? 0 : (t % 4 == 1 ? 3 : lrmf_lds_rows(16)));
    }
    {   // the empty matrix; a single user; all users on one item; disjoint users
        Csr e;
        e.ptr.assign(4, 0);
        check(e, 3, 5, lrmf_lds_rows(4));
        Csr one{{0, 2}, {1, 4}, {2.0, 0.0}};
        check(one, 1, 5, lrmf_lds_rows(4));
        Csr hub, dis;
        hub.ptr.push_back(0), dis.ptr.push_back(0);
        for (int u = 0; u < 50; ++u) {
            hub.idx.push_back(0), hub.val.push_back(1.0 + u % 3), hub.ptr.push_back(u + 1);
            dis.idx.push_back(u), dis.val.push_back(2.0), dis.ptr.push_back(u + 1);
        }
        check(hub, 50, 1, lrmf_lds_rows(4));
        check(dis, 50, 50, lrmf_lds_rows(4));
    }
    {   // a large one: 20 000 users x 3 000 items
        const Csr m = random_matrix(rng, 20000, 3000, 30);
        check(m, 20000, 3000, lrmf_lds_rows(64));
    }
    for (int k = 1; k <= LRMF_MAX_K; ++k) CHECK(lrmf_lds_bytes(k, lrmf_lds_rows(k)) <= (size_t)LRMF_LDS_BYTES && lrmf_lds_rows(k) >= LRMF_BLOCK / 2);
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("lrmf host checks passed\n");
    return failures ? 1 : 0;
}
