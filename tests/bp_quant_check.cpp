// The broad phase's quantiser (d3d12renderer_amd/csrc/bp_quant.hpp) on the host: for random box pairs on random frames, every pair the exact closed-interval test
// accepts must pass the quantised test.  Built and run by tests/test_bp_quant.py; prints one line and returns non-zero on a violation.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include "../d3d12renderer_amd/csrc/bp_quant.hpp"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }
static float uni() { return (float)(rnd() >> 40) / 16777216.f; }                       // [0, 1)
static float uni(float lo, float hi) { return lo + (hi - lo) * uni(); }
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

static const float kInf = std::numeric_limits<float>::infinity(), kNaN = std::numeric_limits<float>::quiet_NaN(), kDenorm = 1.0e-41f;

// bounding_volumes.h:352-358 as the pair kernel has it (aabbOverlap): closed intervals, a NaN bound rejects nothing
static bool exactOverlap(const float amn[3], const float amx[3], const float bmn[3], const float bmx[3]) {
    for (int a = 0; a < 3; ++a) if (amx[a] < bmn[a] || amn[a] > bmx[a]) return false;
    return true;
}

struct Box { float mn[3], mx[3]; };

int main(int argc, char** argv) {
    const long pairsWanted = argc > 1 ? atol(argv[1]) : 1200000;
    long pairs = 0, exact = 0, quant = 0, violations = 0, nanPairs = 0;
    while (pairs < pairsWanted) {
        // a frame: mostly a plausible grid, sometimes degenerate
        float origin[3]; uint32_t dims[3]; float cell = expf(uni(-7.f, 7.f));
        for (int a = 0; a < 3; ++a) { origin[a] = uni(-1.0e4f, 1.0e4f); dims[a] = 1u + below(2000u); }
        switch (below(24u)) {
            case 0: cell = 0.f; break;             case 1: cell = kInf; break;       case 2: cell = kNaN; break;          case 3: cell = kDenorm; break;
            case 4: cell = -1.f; break;            case 5: origin[below(3u)] = kInf; break;   case 6: origin[below(3u)] = -kInf; break;   case 7: origin[below(3u)] = kNaN; break;
            case 8: origin[below(3u)] = 3.0e38f; break;   case 9: dims[below(3u)] = 4000000000u; break;   case 10: dims[0] = dims[1] = dims[2] = 1u; break;   case 11: cell = 3.0e38f; break;
            default: break;
        }
        const mi::BpQuantFrame f = mi::bpQuantFrame(origin, dims, cell);
        float lo[3], span[3];
        for (int a = 0; a < 3; ++a) { lo[a] = origin[a] - cell; span[a] = ((float)dims[a] + 2.f) * cell; }
        for (int rep = 0; rep < 256; ++rep, ++pairs) {
            Box A, B;
            const float size = cell * expf(uni(-6.f, 1.f));           // from far below the quantum to a few cells
            for (int a = 0; a < 3; ++a) {
                A.mn[a] = lo[a] + span[a] * uni(-0.05f, 1.05f); A.mx[a] = A.mn[a] + size * uni();
                // the partner: near enough that about half the axes overlap
                B.mn[a] = A.mn[a] + size * uni(-1.5f, 1.5f); B.mx[a] = B.mn[a] + size * uni();
            }
            // special values, each on a random axis / bound
            const uint32_t kind = below(16u), ax = below(3u);
            float* slots[12] = {&A.mn[0], &A.mn[1], &A.mn[2], &A.mx[0], &A.mx[1], &A.mx[2], &B.mn[0], &B.mn[1], &B.mn[2], &B.mx[0], &B.mx[1], &B.mx[2]};
            switch (kind) {
                case 0: B.mn[ax] = A.mx[ax]; break;                                   // faces that coincide exactly
                case 1: B.mx[ax] = A.mn[ax]; break;
                case 2: A.mn[ax] = A.mx[ax] = B.mn[ax] = B.mx[ax]; break;             // equal bounds
                case 3: *slots[below(12u)] = (below(2u) ? kDenorm : -kDenorm); break;
                case 4: *slots[below(12u)] = (below(2u) ? kInf : -kInf); break;
                case 5: *slots[pairs % 12] = kNaN; break;                             // a NaN in each position in turn
                case 6: { const float t = A.mn[ax]; A.mn[ax] = A.mx[ax]; A.mx[ax] = t; } break;   // inverted boxes
                case 7: { const float t = B.mn[ax]; B.mn[ax] = B.mx[ax]; B.mx[ax] = t; } break;
                case 8: *slots[below(12u)] = lo[ax]; break;                           // exactly on the frame's ends ...
                case 9: *slots[below(12u)] = lo[ax] + span[ax]; break;
                case 10: A.mn[ax] = lo[ax] - span[ax]; B.mn[ax] = lo[ax] - 2.f * span[ax]; break;   // ... and beyond them
                case 11: A.mx[ax] = lo[ax] + 2.f * span[ax]; B.mx[ax] = lo[ax] + 3.f * span[ax]; break;
                case 12: A.mn[ax] = -kInf; A.mx[ax] = kInf; break;
                default: break;
            }
            uint32_t ra[4], rb[4];
            mi::bpQuantRow(f, A.mn, A.mx, 1u, ra); mi::bpQuantRow(f, B.mn, B.mx, 2u, rb);
            const bool e = exactOverlap(A.mn, A.mx, B.mn, B.mx), q = mi::bpQuantOverlap(ra, rb);
            if (mi::bpQuantOverlap(rb, ra) != q || ra[3] != 1u || rb[3] != 2u) { ++violations; printf("asymmetric test or lost index at pair %ld\n", pairs); }
            exact += e; quant += q; nanPairs += kind == 5u;
            if (e && !q) {
                if (++violations <= 8) printf("violation: frame origin %g %g %g dims %u %u %u cell %g  A [%g %g %g | %g %g %g]  B [%g %g %g | %g %g %g]\n", origin[0], origin[1], origin[2], dims[0], dims[1], dims[2], cell,
                                              A.mn[0], A.mn[1], A.mn[2], A.mx[0], A.mx[1], A.mx[2], B.mn[0], B.mn[1], B.mn[2], B.mx[0], B.mx[1], B.mx[2]);
            }
        }
    }
    printf("pairs %ld exact_overlaps %ld quantised_passes %ld nan_pairs %ld violations %ld\n", pairs, exact, quant, nanPairs, violations);
    return violations ? 1 : 0;
}
