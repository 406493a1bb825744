/*
 * math_hard_scan.c -- TEST INFRASTRUCTURE: the search behind tests/golden/make_math_hard.py.
 *
 * Finds arguments of om_expf / om_atan2f in the strata described there whose binary64 value (om_expf_f64 / om_atan2f_f64,
 * the value just before the cast to float) lies within `dmax` binary64 ulps of a binary32 round-to-nearest boundary.
 * About one argument in 4000 lies within 65536 ulps and one in 4 * 10^6 within 64, so a fixture needs ~10^9 arguments per
 * stratum: too many for numpy, a few seconds here.  atan2 operand pairs are drawn; exp arguments are walked exhaustively.
 *
 * Everything is integer hashing and IEEE binary64 / binary32 add, mul, div (no libm, build with -ffp-contract=off), and
 * draw i depends on (seed, stratum, i) alone, so the output does not depend on the thread count or on the machine once
 * the caller sorts it by draw index.
 */
#include <stdint.h>
#include <string.h>
#include "oracle_math.h"

static inline uint64_t mh_mix(uint64_t z) {                     /* splitmix64's finaliser */
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
typedef struct { uint64_t s; } mh_rng;
static inline uint64_t mh_next(mh_rng *r) { r->s += 0x9E3779B97F4A7C15ull; return mh_mix(r->s); }
static inline double mh_u01(mh_rng *r) { return (double)(mh_next(r) >> 11) * 0x1p-53; }          /* [0, 1) */
static inline int mh_int(mh_rng *r, int lo, int hi) { return lo + (int)(mh_next(r) % (uint64_t)(hi - lo + 1)); }
static inline float mh_step(float f, int ulps) {                /* f > 0 moved by `ulps` floats */
    uint32_t u; memcpy(&u, &f, 4); u += (uint32_t)ulps; memcpy(&f, &u, 4); return f;
}
static inline int64_t mh_distance(double v) {
    int64_t low = (int64_t)(om_to_bits(v) & 0x1fffffffull) - 0x10000000ll;
    return low < 0 ? -low : low;
}

#define MH_LN2 0x1.62e42fefa39efp-1

/* exp strata: 0 window weights, x in [-12, 0]; 1 the end of the reduction interval, x within 0.0166 of (k + 1/2) ln 2 for
 * k = -115 .. 114; 2 wide, |x| <= 80.  These sets are finite and small against the rarity of the bands (2 * 10^9 floats
 * hold ~160 arguments within 64 ulps), so they are not sampled: mh_scan_exp walks every float. */
static int mh_in_exp_stratum(int stratum, float x) {
    if (stratum == 0) return x >= -12.0f && x <= 0.0f;
    if (stratum == 2) return __builtin_fabsf(x) <= 80.0f;
    double z = (double)x * (1.0 / MH_LN2) - 0.5;               /* x = (z + 1/2) ln 2 */
    double k = om_rint(z);
    double off = (double)x - (k + 0.5) * MH_LN2;
    return k >= -115.0 && k <= 114.0 && off <= 0.0166 && off >= -0.0166;
}

/* atan2 strata: 0 gradient-like, 1 ends of the octant intervals, 2 range edges (inside the guarded range) */
static int mh_draw_atan2(int stratum, mh_rng *r, int64_t i, float *y, float *x) {
    if (stratum == 0) {
        const int s = mh_int(r, 0, 16);                         /* 8 integer bits + s fraction bits: 8..24 significant bits */
        const double q = om_pow2i(s), iq = om_pow2i(-s);
        float p[4];
        for (int j = 0; j < 4; j++) p[j] = (float)((double)(int64_t)(255.0 * q * mh_u01(r) + 0.5) * iq);
        *y = p[0] - p[1];
        *x = p[2] - p[3];
        if (*y == 0.0f || *x == 0.0f) return 0;
    } else if (stratum == 1) {
        const int k = (int)(i % 8), fold = (int)((i >> 3) & 3);
        const double centre = ((double)k + 0.5) * 0.125;
        const float den = (float)(om_pow2i(mh_int(r, -4, 9)) * (1.0 + mh_u01(r)));
        const float num = (float)((centre + (2.0 * mh_u01(r) - 1.0) * 0x1p-10) * (double)den);
        const double off = (double)num / (double)den - centre;
        if (!(off <= 0x1p-10 && off >= -0x1p-10)) return 0;
        const float sy = (mh_next(r) & 1) ? -1.0f : 1.0f, sx = (fold & 2) ? -1.0f : 1.0f;
        *y = sy * ((fold & 1) ? den : num);
        *x = sx * ((fold & 1) ? num : den);
    } else {
        const int which = mh_int(r, 0, 5);
        const int far = (int)(mh_next(r) & 1);
        const double rho = om_pow2i(far ? mh_int(r, -119, -6) : mh_int(r, -5, -1)) * (1.0 + mh_u01(r));   /* min / max */
        float pinned, other;
        if (which < 3) { pinned = mh_step(1e18f, -which); other = (float)((double)pinned * rho); }         /* the larger operand */
        else { pinned = mh_step(1e-18f, which - 3); other = (float)((double)pinned / rho); }               /* the smaller one */
        const uint64_t h = mh_next(r);
        const float a = (h & 1) ? -pinned : pinned, b = (h & 2) ? -other : other;
        if (h & 4) { *y = a; *x = b; } else { *y = b; *x = a; }
        const float ay = __builtin_fabsf(*y), ax = __builtin_fabsf(*x);
        const float mn = ay < ax ? ay : ax;
        if (!(ax <= 1e18f && ay <= 1e18f && mn >= 1e-18f)) return 0;
    }
    return 1;
}

/* Draws i0 .. i0 + n - 1 of atan2 stratum `stratum` (a = y, b = x).  Keeps up to cap arguments with distance <= dmax, in
 * any order, with their draw index; returns how many qualified (may exceed cap). */
int64_t mh_scan_atan2(int stratum, uint64_t seed, int64_t i0, int64_t n, int64_t dmax,
                      float *a, float *b, int64_t *idx, int64_t cap) {
    int64_t count = 0;
    const uint64_t base = mh_mix(mh_mix(seed) + (uint64_t)(16 + stratum));
#pragma omp parallel for schedule(static)
    for (int64_t i = i0; i < i0 + n; i++) {
        mh_rng r = { mh_mix(base + (uint64_t)i) };
        float y = 0.0f, x = 0.0f;
        if (!mh_draw_atan2(stratum, &r, i, &y, &x)) continue;
        if (mh_distance(om_atan2f_f64(y, x)) > dmax) continue;
        int64_t at;
#pragma omp atomic capture
        at = count++;
        if (at < cap) { a[at] = y; b[at] = x; idx[at] = i; }
    }
    return count;
}

/* Every float32 bit pattern in [bits0, bits0 + n) that lies in exp stratum `stratum` with distance <= dmax: the patterns,
 * in any order; returns how many qualified (may exceed cap). */
int64_t mh_scan_exp(int stratum, int64_t bits0, int64_t n, int64_t dmax, uint32_t *bits, int64_t cap) {
    int64_t count = 0;
#pragma omp parallel for schedule(static)
    for (int64_t i = bits0; i < bits0 + n; i++) {
        const uint32_t u = (uint32_t)i;
        float x; memcpy(&x, &u, 4);
        if (!mh_in_exp_stratum(stratum, x)) continue;
        if (mh_distance(om_expf_f64(x)) > dmax) continue;
        int64_t at;
#pragma omp atomic capture
        at = count++;
        if (at < cap) bits[at] = u;
    }
    return count;
}
