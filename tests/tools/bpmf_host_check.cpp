// bpmf_host_check.cpp -- a stand-alone program over the host side of BPMF (carskit_amd/csrc/bpmf_host.hpp: the stream with its cached
// gaussian, Randoms.gamma, the k x k operations, wishart, the hyper-parameter step, the moments, the draw offsets of a Gibbs pass and
// the rounds of the gaussian generator), on random inputs and the edge cases, for a run under AddressSanitizer and
// UndefinedBehaviorSanitizer.  No device:
//
//   hipcc --offload-host-only -x hip -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Icarskit_amd/csrc tests/tools/bpmf_host_check.cpp -o bpmf_host_check && ./bpmf_host_check
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "bpmf_host.hpp"

using namespace cmi;

static int failures = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__);     \
            ++failures;                                             \
        }                                                           \
    } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0 || (std::isnan(a) && std::isnan(b)); }

// the generator's rounds as bpmf_api.cpp runs them, with the device's work done here: attempt t starts 4 t steps after state0; a round
// takes bpmf_gauss_attempts(pairs still needed) attempts; the pairs are numbered across rounds
static std::vector<double> rounds(BpmfStream &st, int64_t n, int *n_rounds) {
    static const JavaLcgJump jump = java_lcg_jump_table();
    std::vector<double> out((size_t)n);
    *n_rounds = 0;
    if (n == 0) return out;
    const int lead = st.have ? 1 : 0;
    const int64_t need = (n - lead + 1) / 2;
    if (lead) out[0] = st.cached;
    if (need == 0) {
        st.have = 0;
        return out;
    }
    const uint64_t state0 = st.state;
    int64_t t0 = 0, pair0 = 0;
    for (;;) {
        const int64_t att = bpmf_gauss_attempts(need - pair0);
        ++*n_rounds;
        int64_t p = pair0;
        for (int64_t t = t0; t < t0 + att; ++t) {
            BpmfStream a;
            a.state = java_lcg_jump(jump, state0, (uint64_t)t * 4u);
            const double v1 = 2.0 * a.nextDouble() - 1.0, v2 = 2.0 * a.nextDouble() - 1.0, s = v1 * v1 + v2 * v2;
            if (!(s < 1.0 && s != 0.0)) continue;
            if (p < need) {
                const double m = std::sqrt(-2.0 * fdlibm_log(s) / s);
                out[(size_t)(lead + 2 * p)] = v1 * m;
                if (lead + 2 * p + 1 < n) out[(size_t)(lead + 2 * p + 1)] = v2 * m;
                if (p == need - 1) {
                    st.state = java_lcg_jump(jump, state0, (uint64_t)(t + 1) * 4u);
                    st.have = lead + 2 * p + 1 < n ? 0 : 1;
                    st.cached = st.have ? v2 * m : 0.0;
                    return out;
                }
            }
            ++p;
        }
        pair0 = p, t0 += att;
    }
}

static void check_stream(std::mt19937_64 &rng) {
    int extended = 0;
    for (int trial = 0; trial < 400; ++trial) {
        BpmfStream a;
        a.state = rng() & JAVA_LCG_MASK;
        if (trial & 1) (void)a.gaussian(); // a cached value at the start
        BpmfStream b = a;
        const int64_t n = trial < 40 ? trial / 4 : (int64_t)(rng() % 700);
        int nr = 0;
        const std::vector<double> got = rounds(b, n, &nr);
        extended += nr > 1;
        for (int64_t t = 0; t < n; ++t) CHECK(same_bits(got[(size_t)t], a.gaussian()));
        CHECK(a.state == b.state && a.have == b.have && (!a.have || same_bits(a.cached, b.cached)));
    }
    CHECK(extended > 0); // some run needed a second round
}

static BpmfMat random_spd(std::mt19937_64 &rng, int n, double ridge) {
    std::normal_distribution<double> nd;
    BpmfMat b((size_t)n * n);
    for (double &x : b) x = nd(rng);
    BpmfMat a = bpmf_mult(b, bpmf_transpose(b, n), n);
    for (int i = 0; i < n; ++i) a[(size_t)i * n + i] += ridge;
    return a;
}

static void check_matrices(std::mt19937_64 &rng) {
    for (int n : {1, 2, 3, 5, 10, 64}) {
        const BpmfMat a = random_spd(rng, n, (double)n);
        BpmfMat L;
        CHECK(bpmf_cholesky(a, n, L));
        const BpmfMat back = bpmf_mult(L, bpmf_transpose(L, n), n);
        for (size_t e = 0; e < a.size(); ++e) CHECK(std::fabs(back[e] - a[e]) <= 1e-9 * (1.0 + std::fabs(a[e])));
        const BpmfMat prod = bpmf_mult(a, bpmf_inv(a, n), n);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) CHECK(std::fabs(prod[(size_t)i * n + j] - (i == j ? 1.0 : 0.0)) <= 1e-8);
    }
    BpmfMat L;
    CHECK(!bpmf_cholesky(BpmfMat{1.0, 2.0, 2.0, 1.0}, 2, L));            // indefinite: null
    CHECK(bpmf_cholesky(BpmfMat{1.0, 1.0, 1.0, 1.0}, 2, L) && L[3] == 0.0); // semidefinite: a zero diagonal, no null
    CHECK(!bpmf_cholesky(BpmfMat{-1.0}, 1, L) && bpmf_cholesky(BpmfMat{0.0}, 1, L) && bpmf_cholesky(BpmfMat{4.0}, 1, L) && L[0] == 2.0);
    CHECK(!bpmf_cholesky(BpmfMat{4.0, 2.0, std::nan(""), 5.0}, 2, L));
    const BpmfMat sing = bpmf_inv(BpmfMat{1.0, 2.0, 2.0, 4.0}, 2); // a singular matrix: the inverse as it stands, no fault
    CHECK(sing.size() == 4);
    CHECK(bpmf_sparse_contains(5, 3) && !bpmf_sparse_contains(5, 4) && bpmf_sparse_contains(8, 7) && !bpmf_sparse_contains(0, 0));
}

static void check_gamma_wishart_hyper(std::mt19937_64 &rng) {
    BpmfStream st;
    st.state = java_lcg_scramble(20261203);
    for (double alpha : {1.0, 1.5, 3.686, 3.7, 13.0, 13.022, 13.1, 50.5, 5000.0}) {
        double sum = 0.0;
        for (int t = 0; t < 400; ++t) {
            const double g = bpmf_gamma(st, alpha, 2.0);
            CHECK(g > 0.0 && std::isfinite(g));
            sum += g;
        }
        CHECK(std::fabs(sum / 400.0 - 2.0 * alpha) < 0.5 * alpha + 1.0); // the mean of gamma(alpha, scale 2)
    }
    CHECK(std::isnan(bpmf_gamma(st, 0.5, 2.0)));
    for (int k : {1, 2, 3, 7, 10, 33}) {
        BpmfMat scale = random_spd(rng, k, (double)k);
        for (double &x : scale) x /= 10.0 * k;
        BpmfMat w;
        CHECK(bpmf_wishart(st, scale, k, (double)(k + 40), w) && w.size() == (size_t)k * k);
        for (size_t e = 0; e < w.size(); ++e) CHECK(std::isfinite(w[e]));
        const BpmfStream before = st;
        BpmfMat bad((size_t)k * k, 0.0);
        bad[0] = -1.0;
        CHECK(!bpmf_wishart(st, bad, k, (double)(k + 40), w) && st.state == before.state && st.have == before.have); // null: no draw
        // a hyper step of a random factor matrix, through the host moments
        const int rows = 5 + k;
        std::normal_distribution<double> nd;
        std::vector<double> X((size_t)rows * k), mean((size_t)k), cov((size_t)k * k), mu((size_t)k, 0.0);
        for (double &x : X) x = nd(rng);
        bpmf_moments_host(X.data(), rows, k, mean.data(), cov.data());
        BpmfMat alpha = bpmf_inv(cov, k);
        bpmf_hyper_side(st, k, rows, mean, cov, alpha, mu);
        for (double x : alpha) CHECK(std::isfinite(x));
        for (double x : mu) CHECK(std::isfinite(x));
    }
    double mean1[2], cov1[4];
    const double one_row[2] = {1.5, -2.0};
    bpmf_moments_host(one_row, 1, 2, mean1, cov1); // rows - 1 == 0: 0 / 0, as the reference
    CHECK(mean1[0] == 1.5 && std::isnan(cov1[0]) && std::isnan(cov1[3]));
}

static void check_rerun(std::mt19937_64 &rng) {
    CHECK(bpmf_rerun_plan({}).slot.empty() && bpmf_rerun_plan({}).taken == 0);
    for (int trial = 0; trial < 300; ++trial) {
        const int n = (int)(rng() % 40);
        std::vector<int32_t> null((size_t)n);
        const unsigned dens = (unsigned)(rng() % 4);
        for (int32_t &f : null) f = dens && rng() % 4 < dens ? 1 : 0;
        if (trial == 0) std::fill(null.begin(), null.end(), 1);
        const BpmfRerun p = bpmf_rerun_plan(null);
        // by definition: slot s's rank = the non-null slots before it; the first launch was right exactly where rank == s
        std::vector<int32_t> want_slot, want_rank;
        int32_t rank = 0;
        for (int s = 0; s < n; ++s) {
            if (null[(size_t)s]) continue;
            if (rank != s) want_slot.push_back(s), want_rank.push_back(rank);
            ++rank;
        }
        CHECK(p.slot == want_slot && p.rank == want_rank && p.taken == rank);
    }
}

int main() {
    std::mt19937_64 rng(20261220);
    check_stream(rng);
    check_matrices(rng);
    check_gamma_wishart_hyper(rng);
    check_rerun(rng);
    if (failures) {
        std::printf("%d bpmf host checks FAILED\n", failures);
        return 1;
    }
    std::printf("bpmf host checks passed\n");
    return 0;
}
