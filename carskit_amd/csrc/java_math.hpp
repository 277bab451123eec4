// java_math.hpp -- the JDK arithmetic that host and device share: StrictMath.exp / StrictMath.log (fdlibm's __ieee754_exp and
// __ieee754_log, restated from the published algorithm) and java.util.Random (the 48-bit LCG, nextInt(bound), a jump-ahead).
// Math.exp / Math.log are only specified to 1 ulp; where it has to choose, the project defines them as StrictMath's.
// Plain C++ for the host layer (host/recommender.hpp), __host__ __device__ under hipcc.  Compile with -ffp-contract=off.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define CMI_JM_HD __host__ __device__
#else
#define CMI_JM_HD
#endif

namespace cmi {

CMI_JM_HD inline uint64_t jm_bits(double x) {
    uint64_t b;
    __builtin_memcpy(&b, &x, 8);
    return b;
}
CMI_JM_HD inline double jm_double(uint64_t b) {
    double x;
    __builtin_memcpy(&x, &b, 8);
    return x;
}
CMI_JM_HD inline double jm_with_high(double x, int32_t hi) { return jm_double(((uint64_t)(uint32_t)hi << 32) | (jm_bits(x) & 0xffffffffULL)); }

// StrictMath.log = fdlibm __ieee754_log, every argument
CMI_JM_HD inline double fdlibm_log(double x) {
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10, two54 = 1.80143985094819840000e+16,
                 Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
                 Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                 Lg7 = 1.479819860511658591e-01;
    uint64_t bits = jm_bits(x);
    int32_t hx = (int32_t)(bits >> 32), k = 0;
    if (hx < 0x00100000) {
        if ((((uint32_t)hx & 0x7fffffffu) | (uint32_t)bits) == 0) return -jm_double(0x7ff0000000000000ULL); // log(+-0) = -inf
        if (hx < 0) return jm_double(0x7ff8000000000000ULL);                                                // log(-#) = NaN
        k -= 54;
        x *= two54; // subnormal: scale up
        bits = jm_bits(x);
        hx = (int32_t)(bits >> 32);
    }
    if (hx >= 0x7ff00000) return x + x;
    k += (hx >> 20) - 1023;
    hx &= 0x000fffff;
    const int32_t i0 = (hx + 0x95f64) & 0x100000;
    x = jm_with_high(x, hx | (i0 ^ 0x3ff00000));
    k += i0 >> 20;
    const double f = x - 1.0, dk = (double)k;
    if ((0x000fffff & (2 + hx)) < 3) {
        if (f == 0.0) return k == 0 ? 0.0 : dk * ln2_hi + dk * ln2_lo;
        const double R = f * f * (0.5 - 0.33333333333333333 * f);
        return k == 0 ? f - R : dk * ln2_hi - ((R - dk * ln2_lo) - f);
    }
    const double s = f / (2.0 + f), z = s * s, w = z * z;
    const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6)), t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
    const double R = t2 + t1;
    if (((hx - 0x6147a) | (0x6b851 - hx)) > 0) {
        const double hfsq = 0.5 * f * f;
        return k == 0 ? f - (hfsq - s * (hfsq + R)) : dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
    }
    return k == 0 ? f - s * (f - R) : dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f);
}

// StrictMath.exp = fdlibm __ieee754_exp, every argument
CMI_JM_HD inline double fdlibm_exp(double x) {
    const double huge = 1.0e+300, twom1000 = 9.33263618503218878990e-302, o_threshold = 7.09782712893383973096e+02,
                 u_threshold = -7.45133219101941108420e+02, ln2HI = 6.93147180369123816490e-01, ln2LO = 1.90821492927058770002e-10,
                 invln2 = 1.44269504088896338700e+00, P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03,
                 P3 = 6.61375632143793436117e-05, P4 = -1.65339022054652515390e-06, P5 = 4.13813679705723846039e-08;
    const uint64_t bits = jm_bits(x);
    uint32_t hx = (uint32_t)(bits >> 32);
    const int xsb = (int)(hx >> 31);
    hx &= 0x7fffffffu;
    double hi = 0.0, lo = 0.0;
    int32_t k = 0;
    if (hx >= 0x40862E42u) { // |x| >= 709.78...
        if (hx >= 0x7ff00000u) {
            if (((hx & 0xfffffu) | (uint32_t)bits) != 0) return x + x; // NaN
            return xsb == 0 ? x : 0.0;                                  // exp(+-inf) = {inf, 0}
        }
        if (x > o_threshold) return huge * huge;
        if (x < u_threshold) return twom1000 * twom1000;
    }
    if (hx > 0x3fd62e42u) {     // |x| > 0.5 ln2
        if (hx < 0x3FF0A2B2u) { // and |x| < 1.5 ln2
            hi = x - (xsb ? -ln2HI : ln2HI);
            lo = xsb ? -ln2LO : ln2LO;
            k = 1 - xsb - xsb;
        } else {
            k = (int32_t)(invln2 * x + (xsb ? -0.5 : 0.5));
            const double t = (double)k;
            hi = x - t * ln2HI;
            lo = t * ln2LO;
        }
        x = hi - lo;
    } else if (hx < 0x3e300000u) { // |x| < 2**-28
        return 1.0 + x;
    }
    const double t = x * x;
    const double c = x - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
    if (k == 0) return 1.0 - ((x * c) / (c - 2.0) - x);
    const double y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi);
    const int32_t hy = (int32_t)(jm_bits(y) >> 32);
    if (k >= -1021) return jm_with_high(y, hy + (int32_t)((uint32_t)k << 20));
    return jm_with_high(y, hy + (int32_t)((uint32_t)(k + 1000) << 20)) * twom1000;
}

// librec's / CARSKit's g(x) = 1 / (1 + Math.exp(-x))
CMI_JM_HD inline double java_logistic(double x) { return 1.0 / (1.0 + fdlibm_exp(-x)); }

// ---- java.util.Random ------------------------------------------------------------------------------------------------------------
constexpr uint64_t JAVA_LCG_A = 0x5DEECE66DULL, JAVA_LCG_C = 0xBULL, JAVA_LCG_MASK = (1ULL << 48) - 1;

CMI_JM_HD inline uint64_t java_lcg_scramble(int64_t seed) { return ((uint64_t)seed ^ JAVA_LCG_A) & JAVA_LCG_MASK; }

// a^(2^b) and the matching sums of c, b = 0 .. 47: state after 2^b draws = A[b] * state + C[b] (mod 2^48)
struct JavaLcgJump {
    uint64_t A[48], C[48];
};
inline JavaLcgJump java_lcg_jump_table() {
    JavaLcgJump t;
    uint64_t a = JAVA_LCG_A, c = JAVA_LCG_C;
    for (int b = 0; b < 48; ++b) {
        t.A[b] = a, t.C[b] = c;
        c = (c * (a + 1)) & JAVA_LCG_MASK;
        a = (a * a) & JAVA_LCG_MASK;
    }
    return t;
}
// the state d draws after `state`: one multiply-add per set bit of d, at most 48
CMI_JM_HD inline uint64_t java_lcg_jump(const JavaLcgJump &t, uint64_t state, uint64_t d) {
    for (int b = 0; b < 48 && d; ++b, d >>= 1)
        if (d & 1) state = (state * t.A[b] + t.C[b]) & JAVA_LCG_MASK;
    return state;
}

// a stream position: next(31) and nextInt(bound) of the published algorithm, its one statement (the host layer's JavaRandom::nextInt
// delegates here); `used` counts the draws taken
struct JavaStream {
    uint64_t state;
    int64_t used;
    CMI_JM_HD int32_t next31() {
        state = (state * JAVA_LCG_A + JAVA_LCG_C) & JAVA_LCG_MASK;
        ++used;
        return (int32_t)(state >> 17);
    }
    // java.util.Random.nextInt(bound), bound > 0: the power-of-two branch, else the rejection loop on bits - val + (bound - 1) < 0
    // (int arithmetic, wrapping).  `cap`: give up (return -1) rather than take a draw past `used == cap`
    CMI_JM_HD int32_t nextInt(int32_t bound, int64_t cap) {
        if (used >= cap) return -1;
        int32_t r = next31();
        const int32_t m = bound - 1;
        if ((bound & m) == 0) return (int32_t)(((int64_t)bound * (int64_t)r) >> 31);
        for (int32_t u = r; (int32_t)((uint32_t)u - (uint32_t)(r = u % bound) + (uint32_t)m) < 0;) {
            if (used >= cap) return -1;
            u = next31();
        }
        return r;
    }
    // java.util.Random.nextDouble(): (((long) next(26) << 27) + next(27)) * 0x1.0p-53, two draws
    CMI_JM_HD double nextDouble() {
        state = (state * JAVA_LCG_A + JAVA_LCG_C) & JAVA_LCG_MASK;
        const int64_t hi = (int64_t)(state >> 22);
        state = (state * JAVA_LCG_A + JAVA_LCG_C) & JAVA_LCG_MASK;
        const int64_t lo = (int64_t)(state >> 21);
        used += 2;
        return (double)((hi << 27) + lo) * 0x1.0p-53;
    }
};

} // namespace cmi
