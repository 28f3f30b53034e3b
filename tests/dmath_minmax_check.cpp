// The reference's min / max / clamp (src/pch.h:57-67, src/core/math.h:30) as the product's d3d12renderer_amd/csrc/dmath.hpp restates them (default) or as the
// oracle's oracle/ora_math.h does (-DCHECK_ORACLE): which argument comes back when the two do not compare, bit for bit, signs of zero included.
// Built and run on the host by tests/test_contact_matrix.py; prints one line per row and returns the number of wrong rows.
#include <cstdio>
#include <cstring>
#include <cstdint>
#include <limits>
#ifdef CHECK_ORACLE
#include "../oracle/ora_math.h"
static float mx(float a, float b) { return ora::fmax2(a, b); }
static float mn(float a, float b) { return ora::fmin2(a, b); }
static float cl(float v, float l, float u) { return ora::clampf(v, l, u); }
static float mx3(float a, float b) { return ora::vmax(ora::vec3(a, a, a), ora::vec3(b, b, b)).y; }
static float mn3(float a, float b) { return ora::vmin(ora::vec3(a, a, a), ora::vec3(b, b, b)).y; }
static float c01(float v) { return ora::clamp01(v); }
#else
#include "../d3d12renderer_amd/csrc/dmath.hpp"
static float mx(float a, float b) { return mi::fmaxr(a, b); }
static float mn(float a, float b) { return mi::fminr(a, b); }
static float cl(float v, float l, float u) { return mi::clampr(v, l, u); }
static float mx3(float a, float b) { return mi::vmax(mi::V3(a), mi::V3(b)).y; }
static float mn3(float a, float b) { return mi::vmin(mi::V3(a), mi::V3(b)).y; }
static float c01(float v) { return mi::clamp01(v); }
#endif

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static bool isNaN(float f) { return (bits(f) & 0x7FFFFFFFu) > 0x7F800000u; }
static int wrong = 0;
// want NaN: any NaN; else the very bits
static void row(const char* what, float got, float want) {
    const bool ok = isNaN(want) ? isNaN(got) : bits(got) == bits(want);
    printf("%-24s got %08x want %08x %s\n", what, bits(got), bits(want), ok ? "ok" : "WRONG");
    wrong += !ok;
}

int main() {
    volatile float zero = 0.f;   // (volatile: the table is computed at run time, by the code the libraries contain)
    const float pz = zero, nz = -zero, nan = zero / zero, one = 1.f;
    row("max(0, NaN) = 0", mx(pz, nan), pz);
    row("max(NaN, 0) = NaN", mx(nan, pz), nan);
    row("max(+0, -0) = +0", mx(pz, nz), pz);
    row("max(-0, +0) = -0", mx(nz, pz), nz);
    row("min(0, NaN) = NaN", mn(pz, nan), nan);
    row("min(NaN, 0) = 0", mn(nan, pz), pz);
    row("clamp(NaN, 0, 1) = 0", cl(nan, pz, one), pz);
    row("clamp(-0, 0, 1) = +0", cl(nz, pz, one), pz);
    // the helpers built on them
    row("clamp01(NaN) = 0", c01(nan), pz);
    row("vmax(0, NaN) = 0", mx3(pz, nan), pz);
    row("vmax(+0, -0) = +0", mx3(pz, nz), pz);
    row("vmin(NaN, 0) = 0", mn3(nan, pz), pz);
    // and ordinary numbers
    row("max(1, 2) = 2", mx(one, 2.f), 2.f);
    row("max(2, 1) = 2", mx(2.f, one), 2.f);
    row("min(1, 2) = 1", mn(one, 2.f), one);
    row("clamp(3, 0, 1) = 1", cl(3.f, pz, one), one);
    row("clamp(-3, 0, 1) = 0", cl(-3.f, pz, one), pz);
    printf("rows wrong %d\n", wrong);
    return wrong;
}
