// mirt_transform (csrc/scene_host.cpp; the arithmetic: scene/scene_xform.hpp, shared with the kernel behind mirt_scene_transform)
// on ranges at both ends of a heap array of exactly n x 15 floats, as a stand-alone program under the address and undefined-
// behaviour sanitizers (built with -ffp-contract=off like the library):
//   1. the rows of the range equal a restatement written here -- per vertex and row of the column-major matrix three products summed
//      left to right, then the translation; the normal normalize(cross(v2 - v0, v1 - v0)) with glm's x * (1 / sqrt(dot)) --, bit for bit;
//   2. the colour of a moved row and every float outside the range keep their bits (a read or write past either end of the
//      allocation is the sanitizer's to report);
//   3. a triangle with v1 == v0 gets a NaN normal;
//   4. n == 0 does nothing (even with a NULL array); a negative n or a NULL argument is MIRT_ERR_INVALID_ARGUMENT.
#include "../../include/mirt.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static float unit()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (float)(rng_state >> 40) * (1.0f / 16777216.0f);
}
static uint32_t bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }

static long long failures = 0;
static void fail(const char *what, int tri, int k)
{
    if (failures++ < 10) std::printf("FAIL %s: triangle %d float %d\n", what, tri, k);
}

static void restate(const float *in, const float *m, const float *tr, float *out)
{
    for (int v = 0; v < 3; v++) {
        const float x = in[3 * v], y = in[3 * v + 1], z = in[3 * v + 2];
        for (int r = 0; r < 3; r++) {
            const float a = m[r] * x, b = m[3 + r] * y, c = m[6 + r] * z;
            const float s = a + b;
            out[3 * v + r] = (s + c) + tr[r];
        }
    }
    float e2[3], e1[3];
    for (int c = 0; c < 3; c++) { e2[c] = out[6 + c] - out[c]; e1[c] = out[3 + c] - out[c]; }
    const float cx = e2[1] * e1[2] - e1[1] * e2[2], cy = e2[2] * e1[0] - e1[2] * e2[0], cz = e2[0] * e1[1] - e1[0] * e2[1];
    const float xx = cx * cx, yy = cy * cy, zz = cz * cz;
    const float d = (xx + yy) + zz;
    const float inv = 1.0f / std::sqrt(d);
    out[9] = cx * inv; out[10] = cy * inv; out[11] = cz * inv;
    out[12] = in[12]; out[13] = in[13]; out[14] = in[14];
}

static void check_range(int n, int first, int count, const float *m, const float *tr, int degenerate_at)
{
    float *a = new float[(size_t)n * 15];                     // exactly the array: the sanitizer guards both ends
    for (int i = 0; i < n * 15; i++) a[i] = 4.0f * unit() - 2.0f;
    if (degenerate_at >= 0) std::memcpy(a + 15 * degenerate_at + 3, a + 15 * degenerate_at, 12);      // v1 = v0
    std::vector<float> before(a, a + (size_t)n * 15);
    const int rc = mirt_transform(a + (size_t)15 * first, count, m, tr);
    if (rc != MIRT_OK) fail("status", first, rc);
    for (int t = 0; t < n; t++) {
        float want[15];
        if (t >= first && t < first + count) restate(&before[(size_t)15 * t], m, tr, want);
        else std::memcpy(want, &before[(size_t)15 * t], sizeof want);
        for (int k = 0; k < 15; k++) {
            const float got = a[15 * t + k];
            if (t == degenerate_at && t >= first && t < first + count && k >= 9 && k < 12) {
                if (!std::isnan(got) || !std::isnan(want[k])) fail("degenerate normal is not NaN", t, k);
            } else if (bits(got) != bits(want[k])) fail(t >= first && t < first + count ? "moved row differs from the restatement" : "row outside the range changed", t, k);
        }
    }
    delete[] a;
}

int main()
{
    const float c = std::cos(0.7f), s = std::sin(0.7f);
    const float yaw[9] = { c, 0.0f, s, 0.0f, 1.01f, 0.0f, -s, 0.0f, c };            // column-major, as Update() builds cameraRot
    const float full[9] = { 0.36f, 0.48f, -0.8f, -0.8f, 0.6f, 0.0f, 0.48f, 0.64f, 0.6f };
    const float tr[3] = { 0.25f, -0.5f, 1.0f }, zero[3] = { 0.0f, 0.0f, 0.0f };
    const int n = 37;
    for (const float *m : { yaw, full })
        for (const float *t : { tr, zero }) {
            check_range(n, 0, 1, m, t, -1);                   // the first triangle alone
            check_range(n, 0, 5, m, t, 2);                    // a range at the front, a degenerate triangle inside
            check_range(n, n - 1, 1, m, t, -1);               // the last triangle alone
            check_range(n, n - 6, 6, m, t, n - 1);            // a range at the end, its last triangle degenerate
            check_range(n, 0, n, m, t, 17);                   // everything
            check_range(n, 11, 0, m, t, 11);                  // nothing
            check_range(1, 0, 1, m, t, -1);
        }
    float one[15] = { 0 };
    if (mirt_transform(nullptr, 0, yaw, tr) != MIRT_OK) fail("n == 0 with a NULL array", 0, 0);
    if (mirt_transform(nullptr, 1, yaw, tr) != MIRT_ERR_INVALID_ARGUMENT) fail("NULL array accepted", 0, 0);
    if (mirt_transform(one, -1, yaw, tr) != MIRT_ERR_INVALID_ARGUMENT) fail("negative n accepted", 0, 0);
    if (mirt_transform(one, 1, nullptr, tr) != MIRT_ERR_INVALID_ARGUMENT) fail("NULL matrix accepted", 0, 0);
    if (mirt_transform(one, 1, yaw, nullptr) != MIRT_ERR_INVALID_ARGUMENT) fail("NULL translation accepted", 0, 0);
    std::printf("%lld failures\n", failures);
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
