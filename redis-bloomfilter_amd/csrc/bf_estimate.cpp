// bf_estimate.cpp — bf_estimate_count: how many distinct keys a filter with X set bits holds.
// Host-only double arithmetic (like bf_optimal_m); no device is touched.
//
// The textbook estimate -(m / k) ln(1 - X / m) assumes every probe uniform on [0, m).  The ruby
// derivation (ruby.rb:51) is not: with R = 2^32 and 32-bit words h, probe i lands on
// (h[i % 2] + i h[..]) % m, so probe 0 is uniform on [0, R) and probe i >= 1 is the sum of
// U[0, R) and U[0, i R), a trapezoid over [0, (i + 1) R), each folded mod m.  The per-bit hit
// rate lambda(b) = sum of the k folded densities is piecewise linear in b, the expected number
// of set bits after n keys is E(n) = integral over [0, m) of 1 - exp(-n lambda(b)), which has a
// closed form per linear piece, and the estimate solves E(n) = X (E is increasing: bisection).
#include "bfhip.h"

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <vector>

namespace {

typedef __int128 i128;
constexpr uint64_t kR = 1ull << 32;

struct Piece {
    double len, lo, d;   // length in bits; the smaller end's rate; larger end's rate - lo (>= 0)
};

i128 ceil_div(i128 a, i128 b) {   // b > 0
    return a >= 0 ? (a + b - 1) / b : -((-a) / b);
}

// Sum over j >= 0 of (alpha + beta x_j), x_j = x4 / 4 + j m, for the x_j inside [c0, c1).
long double fold_segment(i128 x4, i128 m, i128 c0, i128 c1, long double alpha, long double beta) {
    if (c1 <= c0 || x4 >= 4 * c1) return 0.0L;
    i128 j0 = ceil_div(4 * c0 - x4, 4 * m);
    if (j0 < 0) j0 = 0;
    const i128 j1 = ceil_div(4 * c1 - x4, 4 * m) - 1;
    if (j1 < j0) return 0.0L;
    const long double n = (long double)(j1 - j0 + 1);
    const long double x = (long double)x4 / 4.0L;
    return n * alpha + beta * (n * x + (long double)m * ((long double)(j0 + j1) * n / 2.0L));
}

// The density of probe i at bit x4 / 4, folded mod m.
long double folded_density(uint32_t i, i128 x4, i128 m) {
    const long double R = (long double)kR;
    if (i == 0) return fold_segment(x4, m, 0, (i128)kR, 1.0L / R, 0.0L);
    const long double iR = (long double)i * R;
    const i128 c1 = (i128)kR, c2 = (i128)i * kR, c3 = (i128)(i + 1) * kR;
    return fold_segment(x4, m, 0, c1, 0.0L, 1.0L / (R * iR)) +           // rising edge
           fold_segment(x4, m, c1, c2, 1.0L / iR, 0.0L) +                 // plateau (empty for i = 1)
           fold_segment(x4, m, c2, c3, (long double)(i + 1) / iR, -1.0L / (R * iR));   // falling edge
}

std::vector<Piece> rate_pieces(uint64_t m, uint32_t k) {
    std::vector<uint64_t> cut{0, m};
    for (uint32_t i = 0; i < k; ++i)
        for (const i128 c : {(i128)kR, (i128)i * kR, (i128)(i + 1) * kR}) cut.push_back((uint64_t)(c % (i128)m));
    std::sort(cut.begin(), cut.end());
    cut.erase(std::unique(cut.begin(), cut.end()), cut.end());
    std::vector<Piece> out;
    for (size_t p = 0; p + 1 < cut.size(); ++p) {
        const i128 a = cut[p], len = (i128)cut[p + 1] - a;
        // lambda is linear inside the piece: read it at the quarter points (never a breakpoint)
        long double q1 = 0, q3 = 0;
        for (uint32_t i = 0; i < k; ++i) {
            q1 += folded_density(i, 4 * a + len, (i128)m);
            q3 += folded_density(i, 4 * a + 3 * len, (i128)m);
        }
        const double la = (double)std::max(1.5L * q1 - 0.5L * q3, 0.0L);
        const double lb = (double)std::max(1.5L * q3 - 0.5L * q1, 0.0L);
        out.push_back(Piece{(double)len, std::min(la, lb), std::fabs(lb - la)});
    }
    return out;
}

// 1 - (1 - exp(-d)) / d for d >= 0
double one_minus_g(double d) {
    if (d < 1e-3) return d * (0.5 - d * (1.0 / 6.0 - d * (1.0 / 24.0 - d / 120.0)));
    return 1.0 + std::expm1(-d) / d;
}

// E(n): integral of 1 - exp(-n lambda); per piece L (1 - exp(-u) (1 - exp(-d)) / d) with u the
// smaller end's n lambda and d the difference (the integral is symmetric in the two ends).
double expected_bits(const std::vector<Piece>& pieces, double n) {
    double e = 0;
    for (const Piece& p : pieces) {
        const double u = n * p.lo, d = n * p.d;
        e += p.len * (-std::expm1(-u) + std::exp(-u) * one_minus_g(d));
    }
    return e;
}

}  // namespace

extern "C" int bf_estimate_count(uint64_t m_bits, uint32_t k, uint32_t flags, uint64_t set_bits, double* n_hat) {
    if (!n_hat || m_bits == 0 || k == 0 || k > BF_MAX_K || set_bits > m_bits) return BF_EINVAL;
    const bool flat = (flags & (BF_FLAG_ENGINE_MD5 | BF_FLAG_ENGINE_SHA1)) != 0;
    const uint64_t reach = flat ? m_bits : std::min<uint64_t>(m_bits, (uint64_t)k * (kR - 1) + 1);
    if (set_bits == 0) {
        *n_hat = 0.0;
        return BF_OK;
    }
    if (set_bits >= reach) {
        *n_hat = HUGE_VAL;
        return BF_OK;
    }
    if (flat) {
        *n_hat = -((double)m_bits / (double)k) * std::log1p(-(double)set_bits / (double)m_bits);
        return BF_OK;
    }
    const std::vector<Piece> pieces = rate_pieces(m_bits, k);
    const double x = (double)set_bits;
    double lo = 0.0, hi = std::max(1.0, x / (double)k);
    int grow = 0;
    while (expected_bits(pieces, hi) < x) {
        lo = hi;
        hi *= 2.0;
        if (++grow > 1100 || !std::isfinite(hi)) {   // the far tail of the last trapezoid: effectively full
            *n_hat = HUGE_VAL;
            return BF_OK;
        }
    }
    for (int it = 0; it < 200 && hi - lo > 1e-14 * hi; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (expected_bits(pieces, mid) < x) lo = mid; else hi = mid;
    }
    *n_hat = 0.5 * (lo + hi);
    return BF_OK;
}
