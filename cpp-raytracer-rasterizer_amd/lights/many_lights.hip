// many_lights.hip -- hand-written gfx950 kernels around the DirectLight passes of a deferred frame (many_lights.hpp): the planes a
// primary pass left become the records DirectLight reads, and what DirectLight answered becomes pixelColours and the surface's
// words as Draw() computes them (raytracer/Source/raytracer.cpp:583-600) with realSamples == 1.  Both are one lane per pixel and
// bound by their memory traffic: 20 bytes read and 20 written per pixel for the records; 16 read (plus the triangle's colour) and
// up to 16 written for the resolve.  Built with -ffp-contract=off like every kernel of the library.
#include "many_lights.hpp"

namespace mirt {

// closestIntersections[pixel] as a mirt_hit record: position, distance, triangleIndex.  A pixel without a hit carries index -1, which
// DirectLight answers with zeros and never traces.
__global__ __launch_bounds__(256) void k_frame_records(const ManyLightsFrame m)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)m.W * (m.y1 - m.y0)) return;
    const size_t px = (size_t)m.y0 * m.W + (size_t)i;
    uint32_t *h = m.records + (size_t)HIT_WORDS * i;
    const float *p = m.pos + 3 * px;
    h[0] = __float_as_uint(p[0]); h[1] = __float_as_uint(p[1]); h[2] = __float_as_uint(p[2]);
    h[3] = __float_as_uint(m.dist[px]);
    h[4] = (uint32_t)m.index[px];
}

// pixelColours of a pixel that hit triangle i: color = p * (D + indirectLight) (:584-591) added to the zero the pixel's sum starts
// from and divided by realSamples^2 = 1 (:599); a pixel that missed keeps the zero.  Then PutPixelSDL for interior pixels, as the
// frame kernels write them (csrc/rt_kernels.hip): the border keeps its old value.
__global__ __launch_bounds__(256) void k_frame_resolve(const ManyLightsFrame m)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)m.W * (m.y1 - m.y0)) return;
    const size_t px = (size_t)m.y0 * m.W + (size_t)i;
    const int x = (int)(i % m.W), y = m.y0 + (int)(i / m.W);
    const int idx = m.index[px];
    v3 avg = V3(0.0f, 0.0f, 0.0f);
    if (idx >= 0 && idx < m.n) {
        const v3 tcol = ld3(m.tris15 + (size_t)15 * idx + 12);
        const v3 T = add3(ld3(m.direct + 3 * (size_t)i), ld3(m.indirect));
        avg = add3(avg, mul3(tcol, T));
    }
    const v3 out = div3s(avg, 1.0f);
    if (m.rgb) st3(m.rgb + 3 * px, out);
    if (x >= 1 && x < m.W - 1 && y >= 1 && y < m.H - 1)
        m.xrgb[(size_t)(y - m.row_origin) * m.pitch_words + x] = pack_xrgb(out);
}

}  // namespace mirt
