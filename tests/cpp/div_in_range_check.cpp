// Stand-alone host program of tests/test_div_in_range.py: the scale-free division of gymrs_math.h (div_refine, through its host
// emulation div_in_range_emulated) against `/`, the host guard div_in_range_ok of gymrs_physics.h, and the device guard's
// predicate div_num_in_window.  Built with the twin's flags (-O2 -fno-fast-math -ffp-contract=off); prints one JSON object.
//
//   div_in_range_check sweep SEED PAIRS      random (num, den) pairs over the whole window + its edges, reciprocal -1 / 0 / +1 ulp
//   div_in_range_check guard GRAVITY MASSCART MASSPOLE LENGTH FORCE_MAG      the host guard's verdict and interval for one set
//   div_in_range_check window BITS...        div_num_in_window of the given f32 bit patterns (hex)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gymrs_physics.h"

using namespace gymrs;

static uint64_t splitmix(uint64_t& s)
{
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static gymrs_cartpole_params params_of(double gravity, double masscart, double masspole, double length, double force_mag)
{
    gymrs_cartpole_params p;
    std::memset(&p, 0, sizeof(p));
    p.gravity = gravity;
    p.masscart = masscart;
    p.masspole = masspole;
    p.length = length;
    p.force_mag = force_mag;
    p.tau = 0.02;
    p.theta_threshold_radians = 12 * 2 * 3.14159265358979323846 / 360;
    p.x_threshold = 2.4;
    return p;
}

struct Tally {
    uint64_t pairs = 0, mismatches = 0;
    uint32_t first_num = 0, first_den = 0;
    int first_ulps = 0;
    void one(float num, float den)
    {
        const float want = num / den;
        for (int ulps = -1; ulps <= 1; ++ulps) {
            const float got = div_in_range_emulated(num, den, ulps);
            if (f2u(got) != f2u(want)) {
                if (!mismatches) first_num = f2u(num), first_den = f2u(den), first_ulps = ulps;
                ++mismatches;
            }
        }
        ++pairs;
    }
};

static int sweep(uint64_t seed, uint64_t pairs)
{
    Tally t;
    // the ends of the host interval of `den` for the default parameters and two custom sets inside the guard (the sets of
    // tests/test_div_in_range.py and tests/test_gpu_cartpole_fastpath.py), and the ends of the guard's own window
    const gymrs_cartpole_params sets[3] = {params_of(9.8, 1.0, 0.1, 0.5, 10.0), params_of(3.7, 2.5, 0.4, 0.3, 6.0), params_of(24.8, 0.5, 0.3, 1.2, 15.0)};
    float den_edges[6];
    int n_edges = 0;
    for (const auto& p : sets) {
        const CartPoleConsts c = make_consts(p);
        double lo, hi;
        div_den_interval(c, lo, hi);
        if (!div_in_range_ok(c)) {
            std::printf("{\"error\": \"a sweep set fails the host guard\"}\n");
            return 1;
        }
        den_edges[n_edges++] = (float)lo;
        den_edges[n_edges++] = (float)hi;
    }
    const uint32_t n_den_exp = kDivDenExpHi - kDivDenExpLo + 1u, den_man_span = kDivDenManHi - kDivDenManLo + 1u;
    const uint32_t n_exp = kDivNumExpHi - kDivNumExpLo + 1u;
    uint64_t s = seed;
    for (uint64_t i = 0; i < pairs; ++i) {
        const uint64_t r = splitmix(s), q = splitmix(s);
        const uint32_t sign = (uint32_t)(r >> 63) << 31;
        // every 8th numerator on one of the window's edge exponents, every 64th on the very first / very last value of the window
        uint32_t exp = kDivNumExpLo + (uint32_t)((r >> 32) % n_exp), man = (uint32_t)r & 0x7fffffu;
        if ((i & 7u) == 0) exp = (i & 8u) ? kDivNumExpHi : kDivNumExpLo;
        if ((i & 15u) == 1) man = (r & 0x100u) ? 0x7fffffu - (uint32_t)((r >> 12) & 15u) : (uint32_t)((r >> 12) & 15u); // around a power of two
        if ((i & 63u) == 0) man = (i & 8u) ? 0x7fffffu : 0u;
        const float num = u2f(sign | (exp << 23) | man);
        // den: every 5th at an end of a set's host interval; otherwise anywhere in the three binades of the window, every 4th of
        // those within 32 ulps of a binade's window ends
        float den;
        if (i % 5u == 0) {
            den = den_edges[(q >> 40) % (uint64_t)n_edges];
        } else {
            const uint32_t e = kDivDenExpLo + (uint32_t)((q >> 50) % n_den_exp);
            uint32_t m = kDivDenManLo + (uint32_t)(q % den_man_span);
            if ((i & 3u) == 0) m = ((q >> 40) & 1u) ? kDivDenManLo + (uint32_t)(q & 31u) : kDivDenManHi - (uint32_t)(q & 31u);
            den = u2f((e << 23) | m);
        }
        if (!div_den_in_window(den)) {
            std::printf("{\"error\": \"a sweep den outside the window\"}\n");
            return 1;
        }
        t.one(num, den);
    }
    std::printf("{\"pairs\": %" PRIu64 ", \"mismatches\": %" PRIu64 ", \"first\": [\"%08x\", \"%08x\", %d]}\n", t.pairs, t.mismatches, t.first_num,
                t.first_den, t.first_ulps);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 4 && !std::strcmp(argv[1], "sweep")) return sweep(std::strtoull(argv[2], nullptr, 0), std::strtoull(argv[3], nullptr, 0));
    if (argc >= 7 && !std::strcmp(argv[1], "guard")) {
        const CartPoleConsts c = make_consts(params_of(std::atof(argv[2]), std::atof(argv[3]), std::atof(argv[4]), std::atof(argv[5]), std::atof(argv[6])));
        double lo, hi;
        div_den_interval(c, lo, hi);
        std::printf("{\"ok\": %d, \"lo\": \"%.9g\", \"hi\": \"%.9g\"}\n", div_in_range_ok(c) ? 1 : 0, lo, hi);
        return 0;
    }
    if (argc >= 3 && !std::strcmp(argv[1], "window")) {
        std::printf("{\"exp_lo\": %u, \"exp_hi\": %u, \"in\": [", kDivNumExpLo, kDivNumExpHi);
        for (int i = 2; i < argc; ++i) std::printf("%s%d", i > 2 ? ", " : "", div_num_in_window(u2f((uint32_t)std::strtoul(argv[i], nullptr, 16))) ? 1 : 0);
        std::printf("]}\n");
        return 0;
    }
    std::fprintf(stderr, "usage: see the head of the file\n");
    return 2;
}
