// shadow_ray_needed (csrc/rt_common.hpp) on the CPU, and the claim the trace kernel's skip rests on:
//   1. the predicate: false exactly when all three components of D compare equal to zero (+0 or -0 in any mix); true for NaN in any
//      component, infinities, denormals and ordinary values;
//   2. for every D it calls unneeded, `result += D` (raytracer.cpp:319) leaves the very bits that `result += (0, 0, 0)` leaves --
//      what an occluder would have made of D (:313-314) -- for result = +0 (where it starts), for ordinary sums, infinities and
//      NaN; and a result that is never -0 stays so: no chain of such sums from +0 produces -0;
//   3. for every D it calls needed, some component differs in bits from +0: a ray whose answer could change the frame is kept.
#include "../../cpp-raytracer-rasterizer_amd/csrc/rt_common.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

using namespace mirt;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { if (failures++ < 10) std::printf("FAIL line %d: %s\n", __LINE__, #cond); } } while (0)

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
// (volatile: the sums are made at run time, in IEEE single precision, not folded)
static float sum(float a, float b) { volatile float x = a, y = b; volatile float r = x + y; return r; }

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float den = std::numeric_limits<float>::denorm_min(), tiny = std::numeric_limits<float>::min(), big = std::numeric_limits<float>::max();
    const float zeros[2] = { 0.0f, -0.0f };
    const float others[] = { nan, -nan, from_bits(0x7fa00001u) /* signalling */, inf, -inf, den, -den, tiny, -tiny, 1.0f, -1.0f, 0.37f, -2.5e-9f, big, -big };
    const float results[] = { 0.0f, den, -den, tiny, 1.0f, -1.0f, 0.1f, 3.25f, -7.5e-12f, 1.0e30f, big, -big, inf, -inf, nan };
    int cases = 0;

    // 1 + 2: the eight mixes of signed zeros are unneeded, and adding them is adding +0
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2; b++)
            for (int c = 0; c < 2; c++) {
                const float D[3] = { zeros[a], zeros[b], zeros[c] };
                CHECK(!shadow_ray_needed(D[0], D[1], D[2]));
                for (float r : results)
                    for (int i = 0; i < 3; i++) {
                        const float with_d = sum(r, D[i]), with_zero = sum(r, 0.0f);
                        CHECK(bits(with_d) == bits(with_zero) || (std::isnan(with_d) && std::isnan(with_zero) && bits(with_d) == bits(with_zero)));
                        CHECK(bits(with_d) != 0x80000000u);           // never -0 ...
                        // ... so the next light's sum starts from a value this argument covers again
                        CHECK(bits(sum(with_d, D[(i + 1) % 3])) == bits(sum(with_zero, 0.0f)));
                        cases++;
                    }
            }
    // (the one sum that would show the sign: -0 + -0 = -0, which needs a result of -0 -- excluded above)
    CHECK(bits(sum(-0.0f, -0.0f)) == 0x80000000u && bits(sum(0.0f, -0.0f)) == 0u && bits(sum(-0.0f, 0.0f)) == 0u);

    // 1 + 3: anything else in any component keeps the ray, whatever the other two hold
    for (float x : others)
        for (int at = 0; at < 3; at++)
            for (int a = 0; a < 2; a++)
                for (int b = 0; b < 2; b++) {
                    float D[3] = { zeros[a], zeros[b], zeros[a ^ b] };
                    D[at] = x;
                    CHECK(shadow_ray_needed(D[0], D[1], D[2]));
                    CHECK(bits(D[0]) != 0u || bits(D[1]) != 0u || bits(D[2]) != 0u);
                    cases++;
                }
    for (float x : others)
        for (float y : others) {
            CHECK(shadow_ray_needed(x, y, 0.0f) && shadow_ray_needed(-0.0f, x, y) && shadow_ray_needed(y, 0.0f, x) && shadow_ray_needed(x, y, x));
            cases++;
        }
    // a NaN D is what an occluder turns into 0 -- result + NaN is NaN, result + 0 is not: the ray matters
    CHECK(std::isnan(sum(1.0f, nan)) && !std::isnan(sum(1.0f, 0.0f)));

    // how D comes about (raytracer.cpp:304): B * max(dot, 0).  A face turned away: +0 under a positive B, -0 under a negative one, +-0
    // under B = 0 -- all unneeded; B = 0 with the NaN of a light at distance 0 is needed
    const float Bs[] = { 0.75f, -0.75f, 0.0f, -0.0f, den, inf };
    for (float B : Bs) {
        volatile float clamp = 0.0f, Bv = B;
        const float D = Bv * clamp;
        CHECK(shadow_ray_needed(D, D, D) == std::isnan(D));           // (inf * 0 is NaN: kept)
        cases++;
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok: %d cases\n", cases);
    return 0;
}
