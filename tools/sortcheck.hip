// tools/sortcheck.hip -- the bucket sort (csrc/bin_bucket_sort.hip: k_bs_scatter, k_bs_local) and the device-wide exclusive scan
// (csrc/scan.hpp, kernels in csrc/raster_kernels.hip) on their own, against a host counting sort and a host prefix sum.  The two
// sources are INCLUDED below as they are: what runs here is the library's kernel text under the library's flags.
//
//   sortcheck --selftest   no HIP call: builds correct outputs on the host, hands verify_sort / verify_scan one corruption at a time and
//                          requires each to be reported; checks bucket_sort_shift / bucket_sort_buckets over every nbins they can be asked.
//   sortcheck              (GPU box) every nbins of the change-over table x the key patterns below, call variations, an overflowed list,
//                          then the scan on both sides of 1024 and of 1024 x 1024.  One stream, one set of arrays; bucket_cnt and cursor
//                          are zeroed ONCE, before the first case: after that every case starts from what the sort before it left there.
//
// The value of a pair is its own position in the unsorted list, so the check is exact although the order inside a bin is free.
// Everything compared is an integer compared for equality.  Exit code 1 on any violation, 2 on a HIP error (the run stops there).
#include "../cpp-raytracer-rasterizer_amd/csrc/bin_bucket_sort.hip"
#include "../cpp-raytracer-rasterizer_amd/csrc/raster_kernels.hip"
#include "../cpp-raytracer-rasterizer_amd/capi/cube_plan.hpp"          // BIN_MAX_KEYS

#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

namespace {

constexpr uint32_t PATTERN = 0xA5A5A5A5u;       // what every output word holds before a call (no offset, index or count can equal it)
constexpr int PATTERN_BYTE = 0xA5;
constexpr size_t MARGIN = 4096;                  // guard words behind the used part of every array
constexpr uint32_t CAP_PAIRS = 1u << 20;         // pairs the pair arrays hold (4 MiB each)

struct Table { uint32_t nbins; int shift; uint32_t buckets; };
const Table TABLE[] = { { 1, 4, 1 }, { 16, 4, 2 }, { 8191, 4, 512 }, { 16383, 5, 512 }, { 24576, 5, 769 }, { 130000, 7, 1016 }, { 131071, 8, 512 },
                        { 262143, 8, 1024 }, { 262144, 9, 513 }, { 1048575, 10, 1024 }, { 1048576, 11, 513 }, { 2097152, 12, 513 },
                        { 4194303, 12, 1024 }, { 4194304, 12, 1025 }, { 8388607, 12, 2048 } };

// ---- the checks: plain host functions ---------------------------------------------------------------------------------------------

enum { G_ENTRIES, G_TMP_KEYS, G_TMP_VALS, G_BIN_OFF, G_BUCKET_CNT, G_CURSOR, G_BUCKET_BASE, G_ARRAYS };

// The inputs of one bucket_sort_pairs call and everything the device holds after it.
struct SortView {
    const uint32_t *keys;            // the unsorted keys, all below nbins; the values were 0 .. total - 1
    uint32_t total;                  // *total_ptr
    uint32_t nbins, nbuckets;
    bool overflow;                   // total > cap: the call must have written nothing but the counters' reset and count_out
    const uint32_t *bin_off;         // bin_off_words of it
    const uint32_t *entries, *tmp_keys, *tmp_vals;      // pair_words of each
    const uint32_t *bucket_cnt, *cursor;                // nbuckets + MARGIN
    const uint32_t *bucket_base;                        // nbuckets + 1 + MARGIN
    size_t pair_words, bin_off_words;                   // total + MARGIN and nbins + 1 + MARGIN at least
    uint32_t count_out, count_want;  // the word count_out pointed at; *total_ptr, or the pattern where the call was given no count_out
};

struct SortBad {
    uint64_t bin_off = 0, bin_total = 0, perm = 0, wrong_bin = 0, bucket_cnt = 0, cursor = 0, base_total = 0, count_out = 0, guard[G_ARRAYS] = {};
    uint64_t guards() const { uint64_t g = 0; for (uint64_t v : guard) g += v; return g; }
    uint64_t all() const { return bin_off + bin_total + perm + wrong_bin + bucket_cnt + cursor + base_total + count_out + guards(); }
};

uint64_t not_pattern(const uint32_t *a, size_t from, size_t to)
{
    uint64_t bad = 0;
    for (size_t i = from; i < to; i++) bad += a[i] != PATTERN;
    return bad;
}

SortBad verify_sort(const SortView &s)
{
    SortBad bad;
    const uint32_t total = s.total, nbins = s.nbins;
    if (!s.overflow) {
        std::vector<uint32_t> ref((size_t)nbins + 1, 0u);                    // the keys' histogram, then its exclusive prefix sum
        for (uint32_t i = 0; i < total; i++) ref[s.keys[i]]++;
        uint32_t run = 0;
        for (uint32_t b = 0; b <= nbins; b++) { const uint32_t c = ref[b]; ref[b] = run; run += c; }
        for (uint32_t b = 0; b <= nbins; b++) bad.bin_off += s.bin_off[b] != ref[b];
        bad.bin_total = s.bin_off[nbins] != total;
        std::vector<uint8_t> seen(total, 0);
        for (uint32_t p = 0; p < total; p++) {
            const uint32_t e = s.entries[p];
            if (e >= total || seen[e]) bad.perm++; else seen[e] = 1;
        }
        for (uint32_t b = 0; b < nbins; b++) {
            const uint32_t lo = s.bin_off[b], hi = s.bin_off[b + 1];
            if (lo > hi || hi > total) { bad.wrong_bin++; continue; }        // no range to walk
            for (uint32_t p = lo; p < hi; p++) bad.wrong_bin += s.entries[p] >= total || s.keys[s.entries[p]] != b;
        }
        bad.base_total = s.bucket_base[s.nbuckets] != total;
    }
    for (uint32_t b = 0; b < s.nbuckets; b++) { bad.bucket_cnt += s.bucket_cnt[b] != 0u; bad.cursor += s.cursor[b] != 0u; }
    bad.count_out = s.count_out != s.count_want;
    const size_t used = s.overflow ? 0 : total;
    bad.guard[G_ENTRIES] = not_pattern(s.entries, used, s.pair_words);
    bad.guard[G_TMP_KEYS] = not_pattern(s.tmp_keys, used, s.pair_words);
    bad.guard[G_TMP_VALS] = not_pattern(s.tmp_vals, used, s.pair_words);
    bad.guard[G_BIN_OFF] = not_pattern(s.bin_off, s.overflow ? 0 : (size_t)nbins + 1, s.bin_off_words);
    bad.guard[G_BUCKET_CNT] = not_pattern(s.bucket_cnt, s.nbuckets, s.nbuckets + MARGIN);
    bad.guard[G_CURSOR] = not_pattern(s.cursor, s.nbuckets, s.nbuckets + MARGIN);
    bad.guard[G_BUCKET_BASE] = not_pattern(s.bucket_base, (size_t)s.nbuckets + 1, (size_t)s.nbuckets + 1 + MARGIN);
    return bad;
}

// The input of one enqueue_exclusive_scan call (counters = { pattern, 1, pattern, pattern } before it) and what the device holds after it.
struct ScanView {
    const uint32_t *in;
    uint32_t n;
    const uint32_t *data;            // n + 1 + MARGIN
    const uint32_t *sums;            // n / SCAN_ITEMS + 2 + MARGIN
    const uint32_t *counters;        // 4
};

struct ScanBad {
    uint64_t data = 0, data_total = 0, counter_total = 0, flag = 0, counters_kept = 0, guard_sums = 0, guard_data = 0;
    uint64_t all() const { return data + data_total + counter_total + flag + counters_kept + guard_sums + guard_data; }
};

ScanBad verify_scan(const ScanView &s)
{
    ScanBad bad;
    uint32_t run = 0;
    for (uint32_t i = 0; i < s.n; i++) { bad.data += s.data[i] != run; run += s.in[i]; }
    bad.data_total = s.data[s.n] != run;
    bad.counter_total = s.counters[0] != run;
    bad.flag = s.counters[1] != 0u;
    bad.counters_kept = (uint64_t)(s.counters[2] != PATTERN) + (s.counters[3] != PATTERN);
    const size_t sums_used = (size_t)s.n / mirt::SCAN_ITEMS + 2;
    bad.guard_sums = not_pattern(s.sums, sums_used, sums_used + MARGIN);
    bad.guard_data = not_pattern(s.data, (size_t)s.n + 1, (size_t)s.n + 1 + MARGIN);
    return bad;
}

// ---- key patterns ---------------------------------------------------------------------------------------------------------------

struct Rng {
    uint64_t s;
    uint32_t next() { s += 0x9e3779b97f4a7c15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return (uint32_t)((z ^ (z >> 31)) >> 16); }
    uint32_t below(uint32_t n) { return (uint32_t)(((uint64_t)next() * n) >> 32); }
};

std::vector<uint32_t> keys_uniform(Rng &r, uint32_t nbins, uint32_t total)
{
    std::vector<uint32_t> k(total);
    for (auto &x : k) x = r.below(nbins);
    return k;
}

// `full` pairs spread over the bins of the bucket that holds bin nbins / 2, a few hundred elsewhere, in random order
std::vector<uint32_t> keys_one_full_bucket(Rng &r, uint32_t nbins, int shift, uint32_t full)
{
    const uint32_t lo = ((nbins / 2) >> shift) << shift, hi = std::min(lo + (1u << shift), nbins);
    std::vector<uint32_t> k;
    for (uint32_t i = 0; i < full; i++) k.push_back(lo + r.below(hi - lo));
    if (hi - lo < nbins)
        for (int i = 0; i < 300; i++) { const uint32_t b = r.below(nbins - (hi - lo)); k.push_back(b < lo ? b : b + (hi - lo)); }
    for (size_t i = k.size(); i > 1; i--) std::swap(k[i - 1], k[r.below((uint32_t)i)]);
    return k;
}

std::vector<uint32_t> keys_heavy_head(Rng &r, uint32_t nbins, uint32_t total)
{
    const uint32_t head = std::max(nbins / 100u, 1u);
    std::vector<uint32_t> k(total);
    for (auto &x : k) x = (r.next() & 1u) ? r.below(head) : r.below(nbins);
    return k;
}

std::vector<uint32_t> keys_even(Rng &r, uint32_t nbins, uint32_t total)
{
    std::vector<uint32_t> k(total);
    for (auto &x : k) x = 2u * r.below((nbins + 1u) / 2u);
    return k;
}

std::vector<uint32_t> keys_ramp(uint32_t nbins, uint32_t total, bool descending)
{
    std::vector<uint32_t> k(total);
    for (uint32_t i = 0; i < total; i++) k[descending ? total - 1 - i : i] = (uint32_t)((uint64_t)i * nbins / total);
    return k;
}

// ---- --selftest: the checks checked, and the bucket sizing, without a device ------------------------------------------------------

// what a correct sort leaves, built with a host counting sort; every array carries its guard words
struct HostSort {
    std::vector<uint32_t> keys, bin_off, entries, tmp_keys, tmp_vals, bucket_cnt, cursor, bucket_base;
    uint32_t nbins, nbuckets, total, count_out;
    bool overflow = false;
    SortView view() const
    {
        return { keys.data(), total, nbins, nbuckets, overflow, bin_off.data(), entries.data(), tmp_keys.data(), tmp_vals.data(), bucket_cnt.data(),
                 cursor.data(), bucket_base.data(), entries.size(), bin_off.size(), count_out, total };
    }
};

HostSort host_sort(const std::vector<uint32_t> &keys, uint32_t nbins, bool overflow = false)
{
    HostSort h;
    const int shift = mirt::bucket_sort_shift(nbins);
    h.keys = keys; h.nbins = nbins; h.nbuckets = mirt::bucket_sort_buckets(nbins); h.total = (uint32_t)keys.size(); h.count_out = h.total; h.overflow = overflow;
    h.bin_off.assign((size_t)nbins + 1 + MARGIN, PATTERN);
    h.entries.assign(keys.size() + MARGIN, PATTERN); h.tmp_keys = h.entries; h.tmp_vals = h.entries;
    h.bucket_cnt.assign(h.nbuckets + MARGIN, PATTERN); h.cursor = h.bucket_cnt;
    h.bucket_base.assign(h.nbuckets + 1 + MARGIN, PATTERN);
    std::fill(h.bucket_cnt.begin(), h.bucket_cnt.begin() + h.nbuckets, 0u);
    std::fill(h.cursor.begin(), h.cursor.begin() + h.nbuckets, 0u);
    if (overflow) return h;
    std::vector<uint32_t> at((size_t)nbins + 1, 0u), per_bucket(h.nbuckets + 1, 0u);
    for (uint32_t k : keys) { at[k]++; per_bucket[k >> shift]++; }
    uint32_t run = 0;
    for (uint32_t b = 0; b <= nbins; b++) { const uint32_t c = at[b]; at[b] = h.bin_off[b] = run; run += c; }
    run = 0;
    for (uint32_t b = 0; b <= h.nbuckets; b++) { h.bucket_base[b] = run; run += per_bucket[b]; }
    for (uint32_t i = 0; i < h.total; i++) { h.entries[at[keys[i]]++] = i; h.tmp_keys[i] = keys[i]; h.tmp_vals[i] = i; }
    return h;
}

struct HostScan {
    std::vector<uint32_t> in, data, sums, counters;
    ScanView view() const { return { in.data(), (uint32_t)in.size(), data.data(), sums.data(), counters.data() }; }
};

HostScan host_scan(const std::vector<uint32_t> &in)
{
    HostScan h;
    const size_t n = in.size();
    h.in = in;
    h.data.assign(n + 1 + MARGIN, PATTERN);
    h.sums.assign(n / mirt::SCAN_ITEMS + 2 + MARGIN, PATTERN);
    uint32_t run = 0;
    for (size_t i = 0; i < n; i++) { if (i % mirt::SCAN_ITEMS == 0) h.sums[i / mirt::SCAN_ITEMS] = run; h.data[i] = run; run += in[i]; }
    h.data[n] = run;
    h.counters = { run, 0u, PATTERN, PATTERN };
    return h;
}

int g_checks = 0, g_failed = 0;
void expect(bool ok, const char *what, const std::string &where)
{
    g_checks++;
    if (!ok) g_failed++;
    printf("selftest: %-58s %-22s %s\n", what, where.c_str(), ok ? "ok" : "FAILED");
}

int check_sizing()
{
    int bad = 0;
    auto one = [&](uint32_t nbins) {
        const int s = mirt::bucket_sort_shift(nbins);
        const uint32_t nb = mirt::bucket_sort_buckets(nbins);
        if (s < 4 || s > 12 || ((uint64_t)nb << s) < (uint64_t)nbins + 1u || nb > mirt::BUCKET_SORT_MAX_BUCKETS) bad++;
    };
    for (uint32_t nbins = 1; nbins <= 300000u; nbins++) one(nbins);
    Rng r = { 7 };
    for (int i = 0; i < 400000; i++) one(1u + r.below(mirt::BIN_MAX_KEYS));
    one(mirt::BIN_MAX_KEYS);
    return bad;
}

int check_table(bool print)
{
    int bad = 0;
    for (const Table &t : TABLE) {
        const int s = mirt::bucket_sort_shift(t.nbins);
        const uint32_t nb = mirt::bucket_sort_buckets(t.nbins);
        const bool ok = s == t.shift && nb == t.buckets;
        if (print || !ok) printf("sizing: nbins=%u shift=%d buckets=%u (pinned: %d, %u) %s\n", t.nbins, s, nb, t.shift, t.buckets, ok ? "ok" : "CHANGED");
        bad += !ok;
    }
    return bad;
}

int selftest()
{
    static_assert(mirt::BIN_MAX_KEYS == 8388607u, "the table's last row is BIN_MAX_KEYS");
    Rng r = { 1 };
    // the clean outputs pass
    struct Case { const char *name; uint32_t nbins; std::vector<uint32_t> keys; };
    std::vector<Case> cases;
    cases.push_back({ "nbins=1,5 pairs", 1u, std::vector<uint32_t>(5, 0u) });
    cases.push_back({ "nbins=16,100 pairs", 16u, keys_uniform(r, 16u, 100) });
    cases.push_back({ "nbins=8191,5000 pairs", 8191u, keys_uniform(r, 8191u, 5000) });
    cases.push_back({ "nbins=24576,0 pairs", 24576u, {} });
    for (const Case &c : cases) expect(verify_sort(host_sort(c.keys, c.nbins).view()).all() == 0, "clean sort output passes", c.name);
    expect(verify_sort(host_sort(cases[2].keys, cases[2].nbins, true).view()).all() == 0, "clean overflowed call passes", cases[2].name);

    // one corruption at a time, on the two cases with pairs in more than one bin
    struct Corruption { const char *name; std::function<void(HostSort &)> apply; std::function<uint64_t(const SortBad &)> reported; };
    std::vector<Corruption> cs;
    cs.push_back({ "two entries swapped across a bin border", [](HostSort &h) {
                      for (uint32_t p = 1; p < h.total; p++)
                          if (h.keys[h.entries[p - 1]] != h.keys[h.entries[p]]) { std::swap(h.entries[p - 1], h.entries[p]); return; } },
                   [](const SortBad &b) { return b.wrong_bin; } });
    cs.push_back({ "one entry duplicated over another", [](HostSort &h) { h.entries[1] = h.entries[0]; }, [](const SortBad &b) { return b.perm; } });
    cs.push_back({ "bin_off inclusive instead of exclusive", [](HostSort &h) { for (uint32_t b = 0; b < h.nbins; b++) h.bin_off[b] = h.bin_off[b + 1]; },
                   [](const SortBad &b) { return b.bin_off; } });
    cs.push_back({ "bin_off[nbins] missing", [](HostSort &h) { h.bin_off[h.nbins] = PATTERN; }, [](const SortBad &b) { return b.bin_total; } });
    cs.push_back({ "one bucket_cnt word left non-zero", [](HostSort &h) { h.bucket_cnt[h.nbuckets - 1] = 1u; }, [](const SortBad &b) { return b.bucket_cnt; } });
    cs.push_back({ "one cursor word left non-zero", [](HostSort &h) { h.cursor[0] = 7u; }, [](const SortBad &b) { return b.cursor; } });
    cs.push_back({ "bucket_base[nbuckets] not the total", [](HostSort &h) { h.bucket_base[h.nbuckets]--; }, [](const SortBad &b) { return b.base_total; } });
    cs.push_back({ "count_out stale", [](HostSort &h) { h.count_out = h.total + 1u; }, [](const SortBad &b) { return b.count_out; } });
    cs.push_back({ "guard word changed: entries[total]", [](HostSort &h) { h.entries[h.total] = 0u; }, [](const SortBad &b) { return b.guard[G_ENTRIES]; } });
    cs.push_back({ "guard word changed: entries, last", [](HostSort &h) { h.entries.back() = 0u; }, [](const SortBad &b) { return b.guard[G_ENTRIES]; } });
    cs.push_back({ "guard word changed: tmp_keys[total]", [](HostSort &h) { h.tmp_keys[h.total] = 3u; }, [](const SortBad &b) { return b.guard[G_TMP_KEYS]; } });
    cs.push_back({ "guard word changed: tmp_vals[total]", [](HostSort &h) { h.tmp_vals[h.total] = 3u; }, [](const SortBad &b) { return b.guard[G_TMP_VALS]; } });
    cs.push_back({ "guard word changed: bin_off[nbins + 1]", [](HostSort &h) { h.bin_off[h.nbins + 1] = h.total; }, [](const SortBad &b) { return b.guard[G_BIN_OFF]; } });
    cs.push_back({ "guard word changed: bin_off, last", [](HostSort &h) { h.bin_off.back() = h.total; }, [](const SortBad &b) { return b.guard[G_BIN_OFF]; } });
    cs.push_back({ "guard word changed: bucket_cnt[nbuckets]", [](HostSort &h) { h.bucket_cnt[h.nbuckets] = 0u; }, [](const SortBad &b) { return b.guard[G_BUCKET_CNT]; } });
    cs.push_back({ "guard word changed: cursor[nbuckets]", [](HostSort &h) { h.cursor[h.nbuckets] = 0u; }, [](const SortBad &b) { return b.guard[G_CURSOR]; } });
    cs.push_back({ "guard word changed: bucket_base[nbuckets + 1]", [](HostSort &h) { h.bucket_base[h.nbuckets + 1] = h.total; },
                   [](const SortBad &b) { return b.guard[G_BUCKET_BASE]; } });
    for (int ci = 1; ci <= 2; ci++)
        for (const Corruption &c : cs) {
            HostSort h = host_sort(cases[ci].keys, cases[ci].nbins);
            c.apply(h);
            expect(c.reported(verify_sort(h.view())) > 0, c.name, cases[ci].name);
        }
    {
        // an overflowed call that wrote after all
        HostSort h = host_sort(cases[2].keys, cases[2].nbins, true);
        h.entries[3] = 3u;
        expect(verify_sort(h.view()).guard[G_ENTRIES] > 0, "overflowed call wrote an entry", cases[2].name);
        h = host_sort(cases[2].keys, cases[2].nbins, true);
        h.bin_off[0] = 0u;
        expect(verify_sort(h.view()).guard[G_BIN_OFF] > 0, "overflowed call wrote bin_off[0]", cases[2].name);
        h = host_sort(cases[2].keys, cases[2].nbins, true);
        h.bucket_cnt[5] = 9u;
        expect(verify_sort(h.view()).bucket_cnt > 0, "overflowed call left a bucket_cnt word", cases[2].name);
        h = host_sort(cases[2].keys, cases[2].nbins, true);
        h.count_out = PATTERN;
        expect(verify_sort(h.view()).count_out > 0, "overflowed call stored no count_out", cases[2].name);
    }

    // the scan
    std::vector<std::pair<const char *, std::vector<uint32_t>>> scans;
    scans.push_back({ "n=1", { 5u } });
    scans.push_back({ "n=1025", std::vector<uint32_t>(1025, 1u) });
    std::vector<uint32_t> rnd(3000);
    for (auto &x : rnd) x = r.below(2561u);
    scans.push_back({ "n=3000", rnd });
    for (auto &s : scans) expect(verify_scan(host_scan(s.second).view()).all() == 0, "clean scan output passes", s.first);
    struct ScanCorruption { const char *name; std::function<void(HostScan &)> apply; std::function<uint64_t(const ScanBad &)> reported; };
    std::vector<ScanCorruption> sc;
    sc.push_back({ "scan: carry off by one at a 1024 boundary", [](HostScan &h) { for (size_t i = 1024; i < h.in.size() && i < 2048; i++) h.data[i]++; },
                   [](const ScanBad &b) { return b.data; } });
    sc.push_back({ "scan: data[n] missing", [](HostScan &h) { h.data[h.in.size()] = PATTERN; }, [](const ScanBad &b) { return b.data_total; } });
    sc.push_back({ "scan: counters[0] not the total", [](HostScan &h) { h.counters[0]++; }, [](const ScanBad &b) { return b.counter_total; } });
    sc.push_back({ "scan: counters[1] left at 1", [](HostScan &h) { h.counters[1] = 1u; }, [](const ScanBad &b) { return b.flag; } });
    sc.push_back({ "scan: counters[2] overwritten", [](HostScan &h) { h.counters[2] = 0u; }, [](const ScanBad &b) { return b.counters_kept; } });
    sc.push_back({ "scan: guard word changed: sums", [](HostScan &h) { h.sums[h.in.size() / mirt::SCAN_ITEMS + 2] = 0u; }, [](const ScanBad &b) { return b.guard_sums; } });
    sc.push_back({ "scan: guard word changed: data[n + 1]", [](HostScan &h) { h.data[h.in.size() + 1] = 0u; }, [](const ScanBad &b) { return b.guard_data; } });
    for (int si = 1; si <= 2; si++)
        for (const ScanCorruption &c : sc) {
            HostScan h = host_scan(scans[si].second);
            c.apply(h);
            expect(c.reported(verify_scan(h.view())) > 0, c.name, scans[si].first);
        }

    expect(check_sizing() == 0, "4 <= shift <= 12, buckets << shift > nbins, buckets <= max", "nbins 1 .. BIN_MAX_KEYS");
    expect(check_table(true) == 0, "shift and bucket count at the pinned change-overs", "15 nbins");
    printf("selftest: %d checks, %d failing\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}

// ---- the device run ---------------------------------------------------------------------------------------------------------------

#define HIP_OK(call)                                                                                                  \
    do {                                                                                                              \
        const hipError_t e_ = (call);                                                                                 \
        if (e_ != hipSuccess) {                                                                                       \
            printf("HIP error: %s (%s, line %d) -- stopping\n", hipGetErrorString(e_), #call, __LINE__);              \
            fflush(stdout);                                                                                           \
            _Exit(2);                                                                                                 \
        }                                                                                                             \
    } while (0)

// what k_bin_pairs does to the bucket counts: it ADDS its pairs to what the sort before it left there
__global__ void k_add_counts(uint32_t *bucket_cnt, const uint32_t *add, uint32_t nbuckets)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < nbuckets) bucket_cnt[b] += add[b];
}

constexpr size_t MAX_BIN_WORDS = (size_t)mirt::BIN_MAX_KEYS + 1 + MARGIN;
constexpr size_t MAX_BUCKET_WORDS = (size_t)mirt::BUCKET_SORT_MAX_BUCKETS + 1 + MARGIN;
constexpr size_t PAIR_WORDS = (size_t)CAP_PAIRS + MARGIN;
constexpr size_t SCAN_MAX_N = 2500000;

struct Dev {
    hipStream_t stream;
    int cus;
    uint32_t *keys, *vals, *total, *tmp_keys, *tmp_vals, *entries, *bin_off, *bucket_cnt, *bucket_base, *cursor, *add;      // device
    uint32_t *h_count, *d_count;                                                                                             // one pinned word and its device address
    uint32_t *h_bin_off, *h_entries, *h_tmp_keys, *h_tmp_vals, *h_bucket_cnt, *h_cursor, *h_bucket_base;                    // pinned copies
    uint32_t *data, *sums, *counters, *h_data, *h_sums;                                                                      // the scan's
};

template <class T>
void dev_alloc(T **p, size_t words) { HIP_OK(hipMalloc((void **)p, words * sizeof(uint32_t))); }
template <class T>
void host_alloc(T **p, size_t words) { HIP_OK(hipHostMalloc((void **)p, words * sizeof(uint32_t), hipHostMallocDefault)); }

void dev_init(Dev &d)
{
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, 0));
    d.cus = prop.multiProcessorCount;
    HIP_OK(hipStreamCreate(&d.stream));
    dev_alloc(&d.keys, CAP_PAIRS); dev_alloc(&d.vals, CAP_PAIRS); dev_alloc(&d.total, 1);
    dev_alloc(&d.tmp_keys, PAIR_WORDS); dev_alloc(&d.tmp_vals, PAIR_WORDS); dev_alloc(&d.entries, PAIR_WORDS);
    dev_alloc(&d.bin_off, MAX_BIN_WORDS);
    dev_alloc(&d.bucket_cnt, MAX_BUCKET_WORDS); dev_alloc(&d.bucket_base, MAX_BUCKET_WORDS); dev_alloc(&d.cursor, MAX_BUCKET_WORDS); dev_alloc(&d.add, MAX_BUCKET_WORDS);
    host_alloc(&d.h_count, 1);
    HIP_OK(hipHostGetDevicePointer((void **)&d.d_count, d.h_count, 0));
    host_alloc(&d.h_bin_off, MAX_BIN_WORDS); host_alloc(&d.h_entries, PAIR_WORDS); host_alloc(&d.h_tmp_keys, PAIR_WORDS); host_alloc(&d.h_tmp_vals, PAIR_WORDS);
    host_alloc(&d.h_bucket_cnt, MAX_BUCKET_WORDS); host_alloc(&d.h_cursor, MAX_BUCKET_WORDS); host_alloc(&d.h_bucket_base, MAX_BUCKET_WORDS);
    dev_alloc(&d.data, SCAN_MAX_N + 1 + MARGIN); dev_alloc(&d.sums, SCAN_MAX_N / mirt::SCAN_ITEMS + 2 + MARGIN); dev_alloc(&d.counters, 4);
    host_alloc(&d.h_data, SCAN_MAX_N + 1 + MARGIN); host_alloc(&d.h_sums, SCAN_MAX_N / mirt::SCAN_ITEMS + 2 + MARGIN);
    // the values: a pair's own position, the same for every case
    std::vector<uint32_t> iota(CAP_PAIRS);
    for (uint32_t i = 0; i < CAP_PAIRS; i++) iota[i] = i;
    HIP_OK(hipMemcpyAsync(d.vals, iota.data(), sizeof(uint32_t) * CAP_PAIRS, hipMemcpyHostToDevice, d.stream));
    // the ONE time the counters are zeroed from outside
    HIP_OK(hipMemsetAsync(d.bucket_cnt, 0, sizeof(uint32_t) * MAX_BUCKET_WORDS, d.stream));
    HIP_OK(hipMemsetAsync(d.cursor, 0, sizeof(uint32_t) * MAX_BUCKET_WORDS, d.stream));
    HIP_OK(hipStreamSynchronize(d.stream));
}

struct Call {
    int expected_mode = 1;           // 0: expected = 1, 1: expected = total, 2: expected = 64 x total
    bool one_cu = false;             // cu_count 1 (two workgroups) instead of the device's
    bool with_count = true;
    bool overflow = false;           // cap = total - 1
};

int g_sort_cases = 0, g_sort_bad = 0, g_scan_cases = 0, g_scan_bad = 0;
bool g_sort_stopped = false;         // the counters were not what a sort must find: no further sort is launched

void run_sort(Dev &d, const char *name, uint32_t nbins, const std::vector<uint32_t> &keys, const Call &c = Call())
{
    if (g_sort_stopped) return;
    const int shift = mirt::bucket_sort_shift(nbins);
    const uint32_t nbuckets = mirt::bucket_sort_buckets(nbins), total = (uint32_t)keys.size();
    if (total > CAP_PAIRS || nbins > mirt::BIN_MAX_KEYS || nbuckets > mirt::BUCKET_SORT_MAX_BUCKETS || (c.overflow && total == 0)) {
        printf("sortcheck: case %s does not fit the arrays\n", name);
        _Exit(3);
    }
    const uint32_t cap = c.overflow ? total - 1u : CAP_PAIRS;
    const uint32_t expected = c.expected_mode == 0 ? 1u : c.expected_mode == 1 ? total : 64u * total;
    const int cus = c.one_cu ? 1 : d.cus;
    g_sort_cases++;

    // inputs: the pairs, their number, and the pairs per bucket on top of what the last sort left in bucket_cnt
    std::vector<uint32_t> add(nbuckets, 0u);
    for (uint32_t k : keys) add[k >> shift]++;
    if (total) HIP_OK(hipMemcpyAsync(d.keys, keys.data(), sizeof(uint32_t) * total, hipMemcpyHostToDevice, d.stream));
    HIP_OK(hipMemcpyAsync(d.total, &total, sizeof total, hipMemcpyHostToDevice, d.stream));
    HIP_OK(hipMemcpyAsync(d.add, add.data(), sizeof(uint32_t) * nbuckets, hipMemcpyHostToDevice, d.stream));
    hipLaunchKernelGGL(k_add_counts, dim3((nbuckets + 255) / 256), dim3(256), 0, d.stream, d.bucket_cnt, d.add, nbuckets);
    HIP_OK(hipGetLastError());
    // Counts that are not the keys' own would send the scatter's stores past the pairs' end.  They can only come from a sort that did
    // not clean up -- which its own case has reported -- so look before the launch, and launch no sort on such a state.
    HIP_OK(hipMemcpyAsync(d.h_bucket_cnt, d.bucket_cnt, sizeof(uint32_t) * nbuckets, hipMemcpyDeviceToHost, d.stream));
    HIP_OK(hipMemcpyAsync(d.h_cursor, d.cursor, sizeof(uint32_t) * nbuckets, hipMemcpyDeviceToHost, d.stream));
    HIP_OK(hipStreamSynchronize(d.stream));
    uint64_t dirty = 0;
    for (uint32_t b = 0; b < nbuckets; b++) dirty += (d.h_bucket_cnt[b] != add[b]) + (d.h_cursor[b] != 0u);
    if (dirty) {
        printf("sort  nbins=%u shift=%d buckets=%u total=%u %s: %llu counter words are not as the sort before this one had to leave them -- no further sort is run\n",
               nbins, shift, nbuckets, total, name, (unsigned long long)dirty);
        g_sort_bad++;
        g_sort_stopped = true;
        return;
    }

    // every output word carries the pattern (the counters: only behind their used part)
    const size_t pair_words = (size_t)total + MARGIN, bin_words = (size_t)nbins + 1 + MARGIN, base_words = (size_t)nbuckets + 1 + MARGIN;
    HIP_OK(hipMemsetAsync(d.entries, PATTERN_BYTE, sizeof(uint32_t) * pair_words, d.stream));
    HIP_OK(hipMemsetAsync(d.tmp_keys, PATTERN_BYTE, sizeof(uint32_t) * pair_words, d.stream));
    HIP_OK(hipMemsetAsync(d.tmp_vals, PATTERN_BYTE, sizeof(uint32_t) * pair_words, d.stream));
    HIP_OK(hipMemsetAsync(d.bin_off, PATTERN_BYTE, sizeof(uint32_t) * bin_words, d.stream));
    HIP_OK(hipMemsetAsync(d.bucket_base, PATTERN_BYTE, sizeof(uint32_t) * base_words, d.stream));
    HIP_OK(hipMemsetAsync(d.bucket_cnt + nbuckets, PATTERN_BYTE, sizeof(uint32_t) * MARGIN, d.stream));
    HIP_OK(hipMemsetAsync(d.cursor + nbuckets, PATTERN_BYTE, sizeof(uint32_t) * MARGIN, d.stream));
    *d.h_count = PATTERN;

    HIP_OK(mirt::bucket_sort_pairs(d.keys, d.vals, d.total, cap, expected, nbins, d.tmp_keys, d.tmp_vals, d.bucket_cnt, d.bucket_base, d.cursor, d.bin_off,
                                   d.entries, cus, d.stream, c.with_count ? d.d_count : nullptr));
    HIP_OK(hipStreamSynchronize(d.stream));

    HIP_OK(hipMemcpyAsync(d.h_entries, d.entries, sizeof(uint32_t) * pair_words, hipMemcpyDeviceToHost, d.stream));
    HIP_OK(hipMemcpyAsync(d.h_tmp_keys, d.tmp_keys, sizeof(uint32_t) * pair_words, hipMemcpyDeviceToHost, d.stream));
    HIP_OK(hipMemcpyAsync(d.h_tmp_vals, d.tmp_vals, sizeof(uint32_t) * pair_words, hipMemcpyDeviceToHost, d.stream));
    HIP_OK(hipMemcpyAsync(d.h_bin_off, d.bin_off, sizeof(uint32_t) * bin_words, hipMemcpyDeviceToHost, d.stream));
    HIP_OK(hipMemcpyAsync(d.h_bucket_base, d.bucket_base, sizeof(uint32_t) * base_words, hipMemcpyDeviceToHost, d.stream));
    HIP_OK(hipMemcpyAsync(d.h_bucket_cnt, d.bucket_cnt, sizeof(uint32_t) * (nbuckets + MARGIN), hipMemcpyDeviceToHost, d.stream));
    HIP_OK(hipMemcpyAsync(d.h_cursor, d.cursor, sizeof(uint32_t) * (nbuckets + MARGIN), hipMemcpyDeviceToHost, d.stream));
    // the counters a case with more buckets will use: zero again, as they were before this case put the pattern there
    HIP_OK(hipMemsetAsync(d.bucket_cnt + nbuckets, 0, sizeof(uint32_t) * MARGIN, d.stream));
    HIP_OK(hipMemsetAsync(d.cursor + nbuckets, 0, sizeof(uint32_t) * MARGIN, d.stream));
    HIP_OK(hipStreamSynchronize(d.stream));

    const SortView v = { keys.data(), total, nbins, nbuckets, c.overflow, d.h_bin_off, d.h_entries, d.h_tmp_keys, d.h_tmp_vals, d.h_bucket_cnt, d.h_cursor,
                         d.h_bucket_base, pair_words, bin_words, *d.h_count, c.with_count ? total : PATTERN };
    const SortBad bad = verify_sort(v);
    printf("sort  nbins=%u shift=%d buckets=%u total=%u expected=%u cu_count=%d count_out=%s %s%s: bin_off=%llu bin_total=%llu perm=%llu wrong_bin=%llu "
           "bucket_cnt=%llu cursor=%llu base_total=%llu count_out=%llu guards=%llu%s\n",
           nbins, shift, nbuckets, total, expected, cus, c.with_count ? "yes" : "no", name, c.overflow ? " OVERFLOW(cap=total-1)" : "",
           (unsigned long long)bad.bin_off, (unsigned long long)bad.bin_total, (unsigned long long)bad.perm, (unsigned long long)bad.wrong_bin,
           (unsigned long long)bad.bucket_cnt, (unsigned long long)bad.cursor, (unsigned long long)bad.base_total, (unsigned long long)bad.count_out,
           (unsigned long long)bad.guards(), bad.all() ? "  <-- MISMATCH" : "");
    if (bad.all()) g_sort_bad++;
}

void sort_cases(Dev &d)
{
    Rng r = { 2024 };
    char name[96];
    for (const Table &t : TABLE) {
        const uint32_t nbins = t.nbins;
        const int shift = mirt::bucket_sort_shift(nbins);
        run_sort(d, "empty", nbins, {});
        run_sort(d, "one-pair-bin0", nbins, { 0u });
        run_sort(d, "one-pair-last-bin", nbins, { nbins - 1u });
        for (uint32_t total : { 4095u, 4096u, 4097u, 8192u, 8193u }) {
            snprintf(name, sizeof name, "uniform-%u", total);
            run_sort(d, name, nbins, keys_uniform(r, nbins, total));
        }
        const uint32_t one_bin[3] = { 0u, nbins - 1u, nbins / 2u };
        const char *which[3] = { "first", "last", "middle" };
        for (int w = 0; w < 3; w++)
            for (uint32_t total : { 4096u, 4097u, 300000u }) {
                snprintf(name, sizeof name, "one-bin-%s-%u", which[w], total);
                run_sort(d, name, nbins, std::vector<uint32_t>(total, one_bin[w]));
            }
        run_sort(d, "one-bucket-4096-rest-sparse", nbins, keys_one_full_bucket(r, nbins, shift, 4096));
        run_sort(d, "one-bucket-4097-rest-sparse", nbins, keys_one_full_bucket(r, nbins, shift, 4097));
        run_sort(d, "uniform-1000000", nbins, keys_uniform(r, nbins, 1000000));
        run_sort(d, "heavy-head-1000000", nbins, keys_heavy_head(r, nbins, 1000000));
        run_sort(d, "even-bins-200000", nbins, keys_even(r, nbins, 200000));
        run_sort(d, "ascending-200000", nbins, keys_ramp(nbins, 200000, false));
        run_sort(d, "descending-200000", nbins, keys_ramp(nbins, 200000, true));
    }
    // call variations: the grid from a guessed `expected`, two workgroups with many chunks each, no count_out, the same call twice
    for (uint32_t nbins : { 8191u, 262144u, 4194304u, 8388607u }) {
        const std::vector<uint32_t> sets[4] = { keys_uniform(r, nbins, 8193), keys_uniform(r, nbins, 1000000), keys_heavy_head(r, nbins, 1000000),
                                                std::vector<uint32_t>(300000, nbins / 2u) };
        const char *names[4] = { "var-uniform-8193", "var-uniform-1000000", "var-heavy-head-1000000", "var-one-bin-middle-300000" };
        for (int s = 0; s < 4; s++) {
            if (nbins == 8388607u && s != 1) continue;             // (34 MB of offsets a call: the uniform list alone)
            for (int em = 0; em < 3; em++)
                for (int one_cu = 0; one_cu < 2; one_cu++)
                    for (int wc = 1; wc >= 0; wc--) {
                        Call c; c.expected_mode = em; c.one_cu = one_cu != 0; c.with_count = wc != 0;
                        run_sort(d, names[s], nbins, sets[s], c);
                    }
            Call again; again.expected_mode = 2; again.one_cu = true; again.with_count = false;
            snprintf(name, sizeof name, "%s-again", names[s]);
            run_sort(d, name, nbins, sets[s], again);               // the very call the loop ended with
        }
    }
    // a list that overflowed: nothing written but the counters' reset and count_out; then an ordinary call on what it left
    {
        const uint32_t nbins = 262143u;
        const std::vector<uint32_t> k = keys_uniform(r, nbins, 100000);
        Call over; over.overflow = true;
        run_sort(d, "uniform-100000", nbins, k, over);
        run_sort(d, "uniform-100000-after-overflow", nbins, k);
        over.with_count = false;
        run_sort(d, "uniform-100000", nbins, k, over);
        run_sort(d, "uniform-8193-after-overflow", 4194304u, keys_uniform(r, 4194304u, 8193));
    }
}

void run_scan(Dev &d, const char *name, const std::vector<uint32_t> &in)
{
    const uint32_t n = (uint32_t)in.size();
    uint64_t sum = 0;
    for (uint32_t x : in) sum += x;
    if (n == 0 || n > SCAN_MAX_N || sum >> 32) { printf("sortcheck: scan case %s does not fit\n", name); _Exit(3); }
    g_scan_cases++;
    const size_t sums_words = (size_t)n / mirt::SCAN_ITEMS + 2 + MARGIN;
    const uint32_t counters[4] = { PATTERN, 1u, PATTERN, PATTERN };
    uint32_t h_counters[4];
    HIP_OK(hipMemcpyAsync(d.data, in.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, d.stream));
    HIP_OK(hipMemsetAsync(d.data + n, PATTERN_BYTE, sizeof(uint32_t) * (1 + MARGIN), d.stream));
    HIP_OK(hipMemsetAsync(d.sums, PATTERN_BYTE, sizeof(uint32_t) * sums_words, d.stream));
    HIP_OK(hipMemcpyAsync(d.counters, counters, sizeof counters, hipMemcpyHostToDevice, d.stream));
    mirt::enqueue_exclusive_scan(d.data, (int)n, d.sums, d.counters, d.stream);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(d.stream));
    HIP_OK(hipMemcpyAsync(d.h_data, d.data, sizeof(uint32_t) * ((size_t)n + 1 + MARGIN), hipMemcpyDeviceToHost, d.stream));
    HIP_OK(hipMemcpyAsync(d.h_sums, d.sums, sizeof(uint32_t) * sums_words, hipMemcpyDeviceToHost, d.stream));
    HIP_OK(hipMemcpyAsync(h_counters, d.counters, sizeof h_counters, hipMemcpyDeviceToHost, d.stream));
    HIP_OK(hipStreamSynchronize(d.stream));
    const ScanView v = { in.data(), n, d.h_data, d.h_sums, h_counters };
    const ScanBad bad = verify_scan(v);
    printf("scan  n=%u %s total=%llu: data=%llu data_total=%llu counter_total=%llu flag=%llu counters_kept=%llu guard_sums=%llu guard_data=%llu%s\n", n, name,
           (unsigned long long)sum, (unsigned long long)bad.data, (unsigned long long)bad.data_total, (unsigned long long)bad.counter_total,
           (unsigned long long)bad.flag, (unsigned long long)bad.counters_kept, (unsigned long long)bad.guard_sums, (unsigned long long)bad.guard_data,
           bad.all() ? "  <-- MISMATCH" : "");
    if (bad.all()) g_scan_bad++;
}

void scan_cases(Dev &d)
{
    Rng r = { 99 };
    char name[64];
    for (uint32_t n : { 1u, 3u, 1023u, 1024u, 1025u, 4097u, 1048575u, 1048576u, 1048577u, 2500000u }) {
        run_scan(d, "all-zero", std::vector<uint32_t>(n, 0u));
        run_scan(d, "all-one", std::vector<uint32_t>(n, 1u));
        std::vector<uint32_t> v(n);
        for (auto &x : v) x = r.below(2561u);
        run_scan(d, "random-0..2560", v);
        // a single non-zero: at the last index, at 1023 and at 1024 (at the last index where the list ends before that)
        const uint32_t at[3] = { n - 1u, std::min(1023u, n - 1u), std::min(1024u, n - 1u) };
        for (int k = 0; k < 3; k++) {
            std::vector<uint32_t> one(n, 0u);
            one[at[k]] = 2560u;
            snprintf(name, sizeof name, "single-nonzero-at-%u%s", at[k], k == 0 ? "(last)" : "");
            run_scan(d, name, one);
        }
    }
}

double seconds_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

int device_run()
{
    const auto t0 = std::chrono::steady_clock::now();
    int ndev = 0;
    HIP_OK(hipGetDeviceCount(&ndev));
    if (ndev < 1) { printf("sortcheck: no HIP device\n"); return 2; }
    HIP_OK(hipSetDevice(0));
    const int table_bad = check_table(true);
    Dev d;
    dev_init(d);
    const auto t1 = std::chrono::steady_clock::now();
    sort_cases(d);
    const double sort_s = seconds_since(t1);
    const auto t2 = std::chrono::steady_clock::now();
    scan_cases(d);
    const double scan_s = seconds_since(t2);
    printf("sizing: %d of the pinned change-overs changed\n", table_bad);
    printf("sort: %d cases, %d mismatching\n", g_sort_cases, g_sort_bad + table_bad);
    printf("scan: %d cases, %d mismatching\n", g_scan_cases, g_scan_bad);
    printf("time: %.2f s in all (set-up %.2f s, sort cases %.2f s, scan cases %.2f s)\n", seconds_since(t0), std::chrono::duration<double>(t1 - t0).count(), sort_s, scan_s);
    return (g_sort_bad || g_scan_bad || table_bad) ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "--selftest")) return selftest();
    if (argc > 1) { printf("usage: sortcheck [--selftest]\n"); return 64; }
    return device_run();
}
