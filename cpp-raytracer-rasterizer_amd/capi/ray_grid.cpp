// ray_grid.cpp -- arbitrary rays through a cell grid (mirt_set_ray_grid, mirt_get_ray_grid_stats; the kernels: ../grid/ray_grid.hip).
// With the switch on, mirt_intersect* and mirt_occluded* (query.cpp) ask here first: the structure of ../grid/ray_grid.hpp -- cells,
// plane index, every-ray list behind one offset table -- is kept per scene version in g.qrows.grid as the along grid is kept: built on
// the stream of the call that finds it missing, the other streams ordered behind the build by events (along_build_begin / _end), its
// pair list and sort scratch its own, forgotten with the scene version, released in mirt_shutdown.  A call the structure cannot serve
// -- a scene the frame path would not bin, a box no grid is made for, more keys than one sort pass holds, an every-ray list that
// outgrew its share (kept as `gave_up`) -- reports so and is answered by query.cpp's sweep.  mirt_set_query_mode is neither read nor
// written here, and no AUTO rule knows the grid yet.
#include "capi.hpp"

namespace mirt {

// Room for the build's pair list and, behind it, the sort's scratch.
static int grid_pairs_room(RayGridCache &C, size_t cap)
{
    int rc;
    C.cap_pairs = 0;
    if ((rc = dev_realloc(&C.d_keys, cap)) || (rc = dev_realloc(&C.d_vals, cap)) || (rc = dev_realloc(&C.d_tmp_keys, cap)) ||
        (rc = dev_realloc(&C.d_tmp_vals, cap)) || (rc = dev_realloc(&C.d_entries, cap))) return rc;
    C.cap_pairs = (uint32_t)cap;
    return MIRT_OK;
}

// The structure for the current scene in C, built on g.stream unless C holds it (along.cpp: along_ensure is the model): the scene's
// rows, the pairs (sized by a read-back of their counts: 8 bytes of pair and every-ray count -- and the plane index's length beside
// them -- and one sync of this stream, the pass repeated if the list was too small), the sort, the rows in key order.
static int grid_ensure(RayGridCache &C, const GridDesc &desc, bool *built)
{
    int rc;
    *built = false;
    if (C.holds(g.scene_version, g.n)) return MIRT_OK;
    *built = true;
    C.valid = false;
    if ((rc = along_build_begin())) return rc;
    const uint32_t nkeys = desc.nkeys, nbuckets = bucket_sort_buckets(nkeys);
    if (nkeys + 1 > C.cap_keys && (rc = dev_grow(&C.d_off, &C.cap_keys, nkeys + 1, (size_t)nkeys + 1, false))) return rc;
    if (!C.d_counters) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&C.d_counters), 64));
    if (nbuckets + 1 > C.cap_buckets && (rc = dev_grow(&C.d_bucket, &C.cap_buckets, nbuckets + 1, (size_t)3 * (nbuckets + 1), false))) return rc;
    if (!C.cap_pairs && (rc = grid_pairs_room(C, (size_t)g.n * 16 + 4096))) return rc;
    uint32_t *bcnt = C.d_bucket, *bbase = C.d_bucket + C.cap_buckets, *bcur = C.d_bucket + 2 * (size_t)C.cap_buckets;

    GridPairs b;
    b.d = desc;
    b.qrows = g.qrows.d_rows;
    b.n = g.n;
    b.counters = C.d_counters;
    b.bucket_cnt = bcnt;
    b.nbuckets = nbuckets;
    b.bucket_shift = bucket_sort_shift(nkeys);
    uint32_t count[6] = { 0u, 0u, 0u, 0u, 0u, 0u };
    bool wrapped = false;
    for (int attempt = 0; attempt < 2; attempt++) {
        b.keys = C.d_keys; b.vals = C.d_vals; b.cap = C.cap_pairs;
        HIP_TRY(hipMemsetAsync(C.d_counters, 0, 64, g.stream));
        HIP_TRY(hipMemsetAsync(C.d_bucket, 0, sizeof(uint32_t) * 3 * (size_t)C.cap_buckets, g.stream));
        hipLaunchKernelGGL(k_grid_pairs, dim3((unsigned)((g.n + 255) / 256)), dim3(256), sizeof(uint32_t) * nbuckets, g.stream, b);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(g.stream));
        HIP_TRY(hipMemcpy(count, C.d_counters, sizeof count, hipMemcpyDeviceToHost));
        // more pairs than 32 bits count (some 129 000 triangles as large as the scene would do): no structure, the calls sweep
        wrapped = (((unsigned long long)count[5] << 32) | count[4]) != (unsigned long long)count[0];
        if (wrapped || count[0] <= C.cap_pairs) break;
        if (attempt == 1) return fail(MIRT_ERR_HIP, "ray grid: the build produced %u pairs twice with room for %u", count[0], C.cap_pairs);
        if ((rc = grid_pairs_room(C, pairs_after_readback(count[0])))) return rc;
    }
    C.gave_up = wrapped || count[1] > (uint32_t)grid_every_cap(g.n);
    C.nrows = C.nplane = C.nevery = 0;
    if (!C.gave_up) {
        HIP_TRY(bucket_sort_pairs(C.d_keys, C.d_vals, C.d_counters, C.cap_pairs, count[0], nkeys, C.d_tmp_keys, C.d_tmp_vals, bcnt, bbase, bcur,
                                  C.d_off, C.d_entries, g.cu_count, g.stream));
        if (count[0] + 1 > C.cap_rows) {
            const size_t rows = (size_t)count[0] + count[0] / 8 + 1024;
            C.cap_rows = 0;
            if ((rc = dev_realloc(&C.d_rows, rows))) return rc;
            C.cap_rows = (uint32_t)rows;
        }
        C.nrows = count[0]; C.nevery = count[1]; C.nplane = count[2];
        // (row 0 is loaded by every lane with no row left: it is there, and finite, whatever the build filed; d_entries has room for
        // 4096 values at least)
        if (!count[0]) {
            HIP_TRY(hipMemsetAsync(C.d_rows, 0, sizeof(QueryRow), g.stream));
            HIP_TRY(hipMemsetAsync(C.d_entries, 0, sizeof(uint32_t), g.stream));
        } else {
            const GridRows x = { C.d_entries, C.d_counters, g.qrows.d_rows, C.d_rows };
            hipLaunchKernelGGL(k_grid_rows, dim3((unsigned)std::min<uint32_t>((count[0] + 255) / 256, 4096u)), dim3(256), 0, g.stream, x);
            HIP_TRY(hipGetLastError());
        }
    }
    if ((rc = along_build_end())) return rc;
    C.desc = desc;
    C.version = g.scene_version;
    C.n = g.n;
    C.valid = true;
    return MIRT_OK;
}

// What both calls do up to their kernel, on the stream the call has taken: the statistics begin afresh; *binned says whether `frame`
// is ready for a walk kernel.
int grid_begin(const void *d_rays, int nrays, GridFrame *frame, bool *binned)
{
    int rc;
    RayGridCache &C = g.qrows.grid;
    RayGridStats &Q = g.grid_stats;
    memset(&Q.s, 0, sizeof Q.s);
    Q.s.mode_used = MIRT_QUERY_BRUTE;
    Q.stream = g.stream;
    Q.dev = nullptr;
    GridDesc desc;
    const int G = grid_cells_for(g.n);
    *binned = g.scene_finite && grid_keys(G) + 64u <= BIN_MAX_KEYS && grid_make_desc(g.bbox_lo, g.bbox_hi, G, &desc);
    if (!*binned) return MIRT_OK;
    bool built = false;
    if ((rc = grid_ensure(C, desc, &built))) return rc;
    Q.s.source = built ? 1 : 2;
    Q.s.gave_up = C.gave_up ? 1 : 0;
    Q.s.cells = C.desc.G;
    Q.s.plane_bins = C.desc.PB;
    Q.s.offset_bins = C.desc.DB;
    Q.s.pairs = C.nrows;
    Q.s.plane_pairs = C.nplane;
    Q.s.every_rows = C.nevery;
    if (C.gave_up) { *binned = false; return MIRT_OK; }
    Q.s.mode_used = MIRT_QUERY_BINNED;
    if ((rc = query_rows())) return rc;                      // (a held structure: this stream behind the rows' build, once)
    memset(frame, 0, sizeof *frame);
    frame->q = rows_frame(d_rays, nrays, nullptr);
    frame->v.d = C.desc;
    frame->v.off = C.d_off;
    frame->v.rows = C.d_rows;
    frame->v.tri = C.d_entries;
    if (g.profiling) {
        unsigned long long *&d = C.d_stats[g.si];
        if (!d) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), sizeof(unsigned long long) * GSTAT_WORDS));
        HIP_TRY(hipMemsetAsync(d, 0, sizeof(unsigned long long) * GSTAT_WORDS, g.stream));
        Q.dev = frame->stats = d;
    }
    return MIRT_OK;
}

template <class Kernel>
static int grid_launch(Kernel plain, Kernel counting, const GridFrame &f)
{
    hipLaunchKernelGGL(f.stats ? counting : plain, dim3((unsigned)((f.q.nrays + 255) / 256)), dim3(256), 0, g.stream, f);
    HIP_TRY(hipGetLastError());
    return MIRT_OK;
}

int ray_grid_intersect(const void *d_rays, int nrays, void *d_hits, bool *done)
{
    int rc;
    GridFrame f;
    if ((rc = grid_begin(d_rays, nrays, &f, done)) || !*done) return rc;
    f.q.hits = static_cast<uint32_t *>(d_hits);
    return grid_launch(k_grid_closest<false>, k_grid_closest<true>, f);
}

int ray_grid_occluded(const void *d_rays, int nrays, const void *d_max_distance, void *d_occluded, bool *done)
{
    int rc;
    GridFrame f;
    if ((rc = grid_begin(d_rays, nrays, &f, done)) || !*done) return rc;
    f.limit = static_cast<const float *>(d_max_distance);
    f.occluded = static_cast<uint8_t *>(d_occluded);
    return grid_launch(k_grid_occluded<false>, k_grid_occluded<true>, f);
}

static int ray_grid_set(int on)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (on != 0 && on != 1) return fail(MIRT_ERR_INVALID_ARGUMENT, "ray grid switch %d is neither 0 nor 1", on);
    g.ray_grid = on;
    return MIRT_OK;
}

static int ray_grid_get_stats(mirt_ray_grid_stats *out)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (!out) return fail(MIRT_ERR_INVALID_ARGUMENT, "out must not be NULL");
    RayGridStats &Q = g.grid_stats;
    if (Q.stream) HIP_TRY(hipStreamSynchronize(Q.stream));
    if (Q.dev) {
        unsigned long long c[GSTAT_WORDS] = {};
        HIP_TRY(hipMemcpy(c, Q.dev, sizeof c, hipMemcpyDeviceToHost));
        Q.s.rays = c[GSTAT_RAYS];
        Q.s.rows_cells = c[GSTAT_ROWS_CELLS];
        Q.s.rows_planes = c[GSTAT_ROWS_PLANES];
        Q.s.rows_every = c[GSTAT_ROWS_EVERY];
        Q.s.tests = c[GSTAT_TESTS];
        Q.s.swept_rays = c[GSTAT_SWEPT];
        Q.dev = nullptr;                         // (read once: a later call on the stream zeroes the words again)
    }
    *out = Q.s;
    return MIRT_OK;
}

}  // namespace mirt

extern "C" int mirt_set_ray_grid(int on) { return mirt::ray_grid_set(on); }
extern "C" int mirt_get_ray_grid_stats(mirt_ray_grid_stats *out) { return mirt::ray_grid_get_stats(out); }
