// tools/veldiv_check.c — CPU evidence for div2_shared of csrc/step_march.hpp: the two fp32 velocity divisions of a site, ux = mx / rho and
// uy = my / rho, on ONE reciprocal (developer experiment, in the manner of tools/fastdiv_check.c).
//
//   rc = v_rcp_f32(b);  f0 = fma(-b, rc, 1);  f1 = fma(f0, rc, rc)                                            once per denominator
//   mu = a f1;  f2 = fma(-b, mu, a);  f3 = fma(f2, f1, mu);  f4 = fma(-b, f3, a);  q = fma(f4, f1, f3)      per numerator
//
// v_rcp_f32 is accurate to one ulp, which of the floats around 1/b it returns is the hardware's affair.  This program runs the chain with rc set to
// EACH float within one ulp of 1/b (RN(1/b) and its two neighbours) and compares every q with the correctly rounded a / b: no mismatch means the
// result does not depend on the reciprocal the hardware returns.  N pairs (default 10^9) from the two populations of the device self-test
// (k_check_veldiv, option "selftest_veldiv"), the ranges the kernel's guard admits:
//   pseudo-random half: b uniform in significand over the binades of [0.5, 18), a over the binades of [2^-103, 12), both signs;
//   built half: a = RN(q b) -3 .. +3 ulps for q next to rounding midpoints, a = +0, a and b at both ends of their ranges.
//   gcc -O2 -march=native -fopenmp -ffp-contract=off tools/veldiv_check.c -lm -o /tmp/veldiv_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uint64_t mix(uint64_t z) { z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL; z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL; return z ^ (z >> 31); }
static float f_of(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t b_of(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

#define A_MIN 0x0c000000u        // 2^-103: below it v_div_scale_f32 scales
#define A_END 0x41400000u        // 12.0 (excluded)
#define B_MIN 0x3f000000u        // 0.5
#define B_END 0x41900000u        // 18.0 (excluded)

// pair number i of the stream `seed` (the same construction as veldiv_pair in csrc/step_march.hpp)
static void veldiv_pair(uint64_t seed, uint64_t i, float *a, float *b)
{
    const uint64_t z = mix(seed + 0x9e3779b97f4a7c15ULL * (i + 1)), y = mix(z);
    // b: one of the six binades [0.5, 1) .. [16, 32), uniform significand, the last cut at 18
    const uint32_t eb = 126u + (uint32_t)((z >> 23) % 6u);
    uint32_t bb = (eb << 23) | (uint32_t)(z & 0x7fffffu);
    if (bb >= B_END) bb = (eb << 23) | (uint32_t)(z & 0xfffffu);
    const uint32_t sign = (uint32_t)(z >> 63) << 31;
    uint32_t ab;
    if (!(i & 1)) {                                  // pseudo-random: one of the 107 binades 2^-103 .. [8, 16), the last cut at 12
        const uint32_t ea = 24u + (uint32_t)((z >> 32) % 107u);
        ab = (ea << 23) | (uint32_t)(y & 0x7fffffu);
        if (ab >= A_END) ab = (ea << 23) | (uint32_t)(y & 0x3fffffu);
        ab |= sign;
    } else if ((i & 14) == 2) {                      // +0
        ab = 0;
    } else if ((i & 14) == 4) {                      // the ends of both ranges, a few ulps inside
        const uint32_t da = (uint32_t)(y & 7u), db = (uint32_t)((y >> 3) & 7u);
        ab = (((y >> 6) & 1u) ? A_END - 1u - da : A_MIN + da) | sign;
        bb = ((y >> 7) & 1u) ? B_END - 1u - db : B_MIN + db;
    } else {                                         // a = RN(m b) -3 .. +3 ulps, m the midpoint above a float q of [2^e, 2^(e+1)), e = -101 .. -2
        const uint32_t eq = (uint32_t)(26u + (z >> 32) % 100u) << 23;
        const float q = f_of(eq | (uint32_t)(y & 0x7fffffu)), bf = f_of(bb);
        const float xm = fmaf(q, bf, (f_of(eq) * 0x1p-24f) * bf);      // (2^e 2^-24: half an ulp of q; times b: exact)
        ab = (b_of(xm) + (uint32_t)((y >> 60) & 7u) - 3u) | sign;
    }
    *a = f_of(ab);
    *b = f_of(bb);
}

static float chain(float a, float b, float rc)
{
    const float f0 = fmaf(-b, rc, 1.0f), f1 = fmaf(f0, rc, rc);
    const float mu = a * f1, f2 = fmaf(-b, mu, a), f3 = fmaf(f2, f1, mu), f4 = fmaf(-b, f3, a);
    return fmaf(f4, f1, f3);
}

int main(int argc, char **argv)
{
    const long long n = argc > 1 ? atoll(argv[1]) : 1000000000LL;
    const uint64_t seed = argc > 2 ? strtoull(argv[2], 0, 10) : 0x5eedULL;
    long long bad = 0, outside = 0, zeros = 0;
#pragma omp parallel for reduction(+ : bad, outside, zeros) schedule(static)
    for (long long i = 0; i < n; i++) {
        float a, b;
        veldiv_pair(seed, (uint64_t)i, &a, &b);
        const uint32_t aa = b_of(a) & 0x7fffffffu;
        if (!(b_of(a) == 0 || (aa >= A_MIN && aa < A_END)) || b_of(b) < B_MIN || b_of(b) >= B_END) { outside++; continue; }      // (none: counted to show it)
        zeros += b_of(a) == 0;
        const float ref = a / b, r0 = 1.0f / b;
        const float rcs[3] = {nextafterf(r0, 0.0f), r0, nextafterf(r0, 4.0f)};
        for (int k = 0; k < 3; k++) {
            const float q = chain(a, b, rcs[k]);
            if (b_of(q) != b_of(ref)) {
                bad++;
#pragma omp critical
                if (bad < 5) printf("mismatch: a %a b %a rc %a: chain %a, a / b %a\n", a, b, rcs[k], q, ref);
            }
        }
    }
    printf("veldiv: %lld (a, b) pairs (half built: midpoint-hugging quotients, +0 (%lld), range ends; %lld outside the guard's ranges), each with the three "
           "reciprocals within one ulp of 1 / b: %lld mismatches of the shared-reciprocal chain against a / b\n", n, zeros, outside, bad);
    return bad != 0 || outside != 0;
}
