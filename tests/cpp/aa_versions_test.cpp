// The per-pixel state machine of a supersampled frame that shades each carried record once (lights/aa_versions.hpp) on the CPU,
// against a direct restatement of Draw()'s loop (raytracer.cpp:563-600) that runs ClosestIntersection's sequential update on the
// carried record and shades EVERY hit sub-ray.  For realSamples 2 .. 8 and random sub-ray outcomes -- a miss; hits at random
// distances and indices; an exact tie with the carried distance under another index; a hit farther than the carried record; all
// misses; all sub-rays each closer than the last -- it checks that
//   1. a fresh record's closest hit merged by aa_merge leaves the carried record where the sequential sweep leaves it;
//   2. the versions' run counts add up to the hit sub-rays, every version's count is >= 1, and there are at most aa * aa;
//   3. the resolve's additions over the (slot, count) pairs, with the records appended in a shuffled order, give the bits of the
//      reference's sum and of its division by aa * aa;
//   4. x1 / y1 step as the reference's expressions do.
// DirectLight is any pure function of the record's position and index: here a hash of their bits.
#include "../../cpp-raytracer-rasterizer_amd/lights/aa_versions.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace mirt;

#define CHECK(c) do { if (!(c)) { printf("FAILED %s (line %d): aa %d, trial %d, kind %d\n", #c, __LINE__, aa, trial, kind); return 1; } } while (0)

struct Hit { float dist; int index; v3 pos; };

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static bool same3(v3 a, v3 b) { return bits_of(a.x) == bits_of(b.x) && bits_of(a.y) == bits_of(b.y) && bits_of(a.z) == bits_of(b.z); }

// "DirectLight": a pure function of the record, values of mixed magnitude so that the order of the additions shows in the bits
static v3 direct_light(const AaRecord &r)
{
    uint32_t h = 2166136261u;
    const uint32_t w[4] = { bits_of(r.pos.x), bits_of(r.pos.y), bits_of(r.pos.z), (uint32_t)r.index };
    for (uint32_t x : w) { h ^= x; h *= 16777619u; h ^= h >> 13; }
    const float a = (float)(h & 0xffffu) / 65536.0f, b = (float)((h >> 8) & 0xffffu) / 4096.0f, c = (float)(h >> 16) / 1048576.0f;
    return V3(a * 3.0f + 0.001f, b, c * 0.37f);
}

int main()
{
    std::mt19937 rng(20240607u);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    const int NTRI = 40;
    std::vector<v3> colour(NTRI);
    for (v3 &c : colour) c = V3(0.15f + 0.6f * U(rng), 0.15f + 0.6f * U(rng), 0.15f + 0.6f * U(rng));
    const v3 indirect = V3(0.2f, 0.2f, 0.2f);
    long subrays = 0, versions_seen = 0, ties = 0, full = 0;

    for (int aa = 2; aa <= 8; aa++) {
        // 4. the stepping: the reference's own expressions
        for (int c = 0; c < 100; c += 7) {
            int trial = c, kind = -1;
            CHECK(bits_of(aa_sub_start(c, aa)) == bits_of((float)c - 0.5f));
            CHECK(bits_of(aa_sub_step(aa)) == bits_of(1.0f / (float)(aa - 1)));
        }
        for (int trial = 0; trial < 4000; trial++) {
            // kind 0: mixed; 1: all misses; 2: every sub-ray closer than the last; 3: many ties and farther hits
            const int kind = trial % 16 == 1 ? 1 : (trial % 16 == 2 ? 2 : (trial % 4 == 3 ? 3 : 0));
            const int n = aa * aa;
            // the accepted triangles of every sub-ray, in index order (ClosestIntersection's loop order)
            std::vector<std::vector<Hit>> sub(n);
            float last = 100.0f;
            float carried_guess = 50.0f;                       // a distance likely to be the carried one, for ties
            for (int s = 0; s < n; s++) {
                if (kind == 1) continue;
                if (kind == 2) { last *= 0.97f; sub[s].push_back({ last, (int)(rng() % NTRI), V3(U(rng), U(rng), last) }); continue; }
                const int roll = (int)(rng() % 8);
                if (roll == 0) continue;                           // a miss
                const int cnt = 1 + (int)(rng() % 3);
                int idx = (int)(rng() % 8);
                for (int k = 0; k < cnt && idx < NTRI; k++, idx += 1 + (int)(rng() % 12)) {
                    float d;
                    const int how = (int)(rng() % (kind == 3 ? 3 : 6));
                    if (how == 0) d = carried_guess;               // an exact tie with (what may be) the carried distance, another index
                    else if (how == 1) d = carried_guess + 1.0f + U(rng);   // farther than the carried record
                    else d = 1.0f + 60.0f * U(rng);
                    sub[s].push_back({ d, idx, V3(U(rng), U(rng) - 0.5f, d) });
                    if (d < carried_guess) carried_guess = d;
                }
            }

            // ---- the reference: the sequential update on the carried record, every hit sub-ray shaded (:563-600) ----
            AaRecord ref = aa_record_reset();
            v3 avg_ref = V3(0.0f, 0.0f, 0.0f);
            int hit_subrays = 0;
            float x1 = aa_sub_start(11, aa);
            for (int s = 0; s < n; s++) {
                bool any = false;
                for (const Hit &h : sub[s]) {
                    if (ref.dist >= h.dist) { ref.pos = h.pos; ref.dist = h.dist; ref.index = h.index; }   // :243-247
                    any = true;                                    // :251
                }
                if (any) {
                    const v3 D = direct_light(ref);                // :583
                    const v3 T = add3(D, indirect);                // :584-586
                    const v3 R = mul3(colour[ref.index], T);       // :587-588
                    avg_ref = add3(avg_ref, R);                    // :591
                    x1 += 1.0f / (float)(aa - 1);                  // :593
                    hit_subrays++;
                }
            }
            const v3 out_ref = div3s(avg_ref, (float)(aa * aa));   // :599

            // ---- the header: fresh record + merge, versions, run counts; the records land in the list in a shuffled order ----
            AaRecord carried = aa_record_reset();
            AaRuns runs = aa_runs_reset();
            std::vector<AaRecord> version;                         // by version number
            std::vector<int> count;
            float x1h = aa_sub_start(11, aa);
            int hits_h = 0;
            for (int s = 0; s < n; s++) {
                AaRecord fresh = aa_record_reset();
                bool accepted = false;
                for (const Hit &h : sub[s]) {
                    if (fresh.dist >= h.dist) { fresh.pos = h.pos; fresh.dist = h.dist; fresh.index = h.index; }
                    accepted = true;
                }
                const bool was_tie = accepted && carried.index >= 0 && carried.dist == fresh.dist;
                const bool replaced = aa_merge(carried, accepted, fresh);
                if (was_tie) { CHECK(replaced); ties++; }          // a later sub-ray wins an exact tie
                const int ended = runs.count;
                const int ev = aa_sub_event(runs, accepted, replaced);
                if (ev == AA_SUB_BEGIN) {
                    if (runs.nver > 1) count.back() = ended;
                    version.push_back(carried);
                    count.push_back(0);
                }
                if (accepted) { hits_h++; x1h += aa_sub_step(aa); }
                CHECK((ev != AA_SUB_NONE) == accepted);
            }
            if (runs.nver > 0) count.back() = runs.count;
            // 1. the carried record is the sequential sweep's
            CHECK(carried.index == ref.index && bits_of(carried.dist) == bits_of(ref.dist) && same3(carried.pos, ref.pos));
            CHECK(bits_of(x1h) == bits_of(x1) && hits_h == hit_subrays);
            // 2. the runs
            CHECK(runs.nver == (int)version.size() && runs.nver <= n);
            int total = 0;
            for (int c : count) { CHECK(c >= 1); total += c; }
            CHECK(total == hit_subrays);
            if (kind == 1) CHECK(runs.nver == 0 && hit_subrays == 0);
            if (kind == 2) { CHECK(runs.nver == n); full += (n == 64); }
            // 3. the resolve by slot, the list in a shuffled order
            std::vector<int> slot_of(version.size());
            for (size_t v = 0; v < version.size(); v++) slot_of[v] = (int)v;
            for (size_t v = version.size(); v > 1; v--) std::swap(slot_of[v - 1], slot_of[rng() % v]);
            std::vector<AaRecord> list(version.size());
            for (size_t v = 0; v < version.size(); v++) list[slot_of[v]] = version[v];
            v3 avg = V3(0.0f, 0.0f, 0.0f);
            for (size_t v = 0; v < version.size(); v++) {
                const AaRecord &r = list[slot_of[v]];
                avg = aa_resolve_add(avg, colour[r.index], direct_light(r), indirect, count[v]);
            }
            CHECK(same3(avg, avg_ref));
            CHECK(same3(aa_resolve_div(avg, aa), out_ref));
            subrays += n; versions_seen += runs.nver;
        }
    }
    if (ties < 1000 || full < 100 || versions_seen >= subrays) { printf("FAILED: the trials miss their cases (ties %ld, full %ld, versions %ld of %ld)\n", ties, full, versions_seen, subrays); return 1; }
    printf("ok: %ld sub-rays, %ld versions, %ld exact ties, %ld pixels of 64 versions\n", subrays, versions_seen, ties, full);
    return 0;
}
