// aa_plan.hpp -- how a supersampled frame that shades each carried record once (rt_frame.cpp; ../lights/aa_many_lights.hpp) cuts its
// band into chunks of rows: pure arithmetic, free of library state; tests/test_aa_many_lights_host.py checks it on the CPU.
//
// A chunk's record list holds the worst case, every sub-ray of every pixel a version of its own: pixels x aa x aa records.  Per
// record the stream keeps 20 bytes of hit record, 12 of DirectLight's answer, 24 of carry between the passes and 8 of (slot, count);
// per pixel 4 more for its version count.  The rows of a chunk are what a budget of scratch bytes holds, at least one.
#pragma once

#include <algorithm>
#include <cstddef>

namespace mirt {

constexpr long long AA_DEFER_SCRATCH_DEFAULT_MB = 256;   // per stream: the order of the 158 MB a plain deferred 1080p frame takes
constexpr long long AA_DEFER_MAX_RECORDS = 1ll << 28;    // DirectLight counts its records in an int; 20 bytes each index below 2^33

inline long long aa_bytes_per_pixel(int aa) { return (long long)aa * aa * (20 + 12 + 24 + 8) + 4; }

// Rows per chunk of a band of `rows` rows, W wide: forced_rows when positive (MIRT_AA_DEFER_ROWS), else what budget_bytes holds;
// at least 1, at most the band, and never more records than AA_DEFER_MAX_RECORDS (but a single row always).
inline int aa_chunk_rows(int W, int rows, int aa, long long budget_bytes, int forced_rows)
{
    const long long per_row = (long long)W * aa_bytes_per_pixel(aa);
    long long r = forced_rows > 0 ? forced_rows : budget_bytes / per_row;
    r = std::min(r, AA_DEFER_MAX_RECORDS / ((long long)W * aa * aa));
    r = std::max(1ll, std::min(r, (long long)std::max(rows, 1)));
    return (int)r;
}

inline int aa_chunk_count(int y0, int y1, int rows_per_chunk) { return y1 > y0 ? (y1 - y0 + rows_per_chunk - 1) / rows_per_chunk : 0; }

// Chunk c of the band [y0, y1): rows [*cy0, *cy1).
inline void aa_chunk_of(int y0, int y1, int rows_per_chunk, int c, int *cy0, int *cy1)
{
    *cy0 = y0 + c * rows_per_chunk;
    *cy1 = std::min(y1, *cy0 + rows_per_chunk);
}

// Records a chunk of `chunk_rows` rows may append: its list's capacity.
inline size_t aa_chunk_records(int W, int chunk_rows, int aa) { return (size_t)W * (size_t)chunk_rows * (size_t)(aa * aa); }

}  // namespace mirt
