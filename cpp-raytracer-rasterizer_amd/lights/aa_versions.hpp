// aa_versions.hpp -- the per-pixel state machine of a supersampled frame that shades each carried record ONCE (aa_many_lights.hip:
// k_aa_primary, k_aa_resolve; ../capi/rt_frame.cpp) and tests/cpp/aa_versions_test.cpp share: Draw()'s sub-ray stepping
// (raytracer/Source/raytracer.cpp:566-596), the merge of a sub-ray's own closest hit into the record the pixel carries (:243), when
// a new "version" of that record begins, how often each version is shaded, and the order of the additions that make pixelColours
// (:583-600).
//
// The reference never resets closestIntersections[pixel] between a pixel's aa x aa sub-rays, so the carried record only ever moves
// to a hit at least as close, and DirectLight (:265-327) is a pure function of the record's position and triangle index.  Consecutive
// hit sub-rays that shade the same carried record therefore add the same three floats to avgColor: a pixel needs one DirectLight
// per distinct record -- a version --, not one per sub-ray.  Versions are consecutive runs: version v is shaded c_v >= 1 times and
// then never again, so avgColor is the sequential sum "c_0 times R_0, then c_1 times R_1, ...", one addition at a time in that order
// (never c * R: a float sum of c equal terms is not their product), which is bit for bit the reference's sum.
#pragma once

#include "../csrc/mirt_math.hpp"

namespace mirt {

// x1 / y1 of Draw(): the pixel's centre, or half a pixel before it when realSamples > 1 (:566-576), advanced by 1 / (realSamples - 1)
// (:593, :596) -- the operations of csrc/rt_common.hpp's aa_start / aa_step, for host and device.
MIRT_HD float aa_sub_start(int c, int rs) { return rs > 1 ? (float)c - 0.5f : (float)c; }
MIRT_HD float aa_sub_step(int rs) { return 1.0f / (float)(rs - 1); }

// closestIntersections[pixel] (struct Intersection, :91-96).  aa_record_reset: Update()'s reset (:335-339), once per frame; it is
// also the fresh record a sub-ray's own closest hit is searched from.
struct AaRecord { float dist; int index; v3 pos; };
MIRT_HD AaRecord aa_record_reset()
{
    AaRecord r;
    r.dist = 3.402823466e+38f; r.index = -1; r.pos = V3(0.0f, 0.0f, 0.0f);
    return r;
}

// One ClosestIntersection call on the carried record, from the call's result on a FRESH record: `accepted` is its return value
// ("some triangle was accepted", :251), `fresh` the closest accepted hit under the sequential rule (smallest distance, latest index
// among equals).  The sequential `carried.distance >= distance` sweep (:243) leaves the carried record at `fresh` exactly when
// carried.distance >= fresh.distance -- a later sub-ray wins an exact tie --, and untouched otherwise; a fresh record nothing
// replaced (its distance still FLT_MAX under index -1: only distances that are not finite do that) replaces nothing.
// Returns whether the carried record was replaced.
MIRT_HD bool aa_merge(AaRecord &carried, bool accepted, const AaRecord &fresh)
{
    if (accepted && fresh.index >= 0 && carried.dist >= fresh.dist) { carried = fresh; return true; }
    return false;
}

// The runs of one pixel.  nver: versions begun so far; count: how often the open version (nver - 1) has been shaded.
struct AaRuns { int nver, count; };
MIRT_HD AaRuns aa_runs_reset() { AaRuns r; r.nver = 0; r.count = 0; return r; }

// What a sub-ray does to the runs.  A sub-ray that was not accepted shades nothing (and x1 does not advance).  An accepted one
// shades the carried record: a new version begins when the merge replaced the record -- or when the pixel has no version yet,
// which takes an accepted sub-ray that replaced nothing, i.e. distances that are not finite: the version is then the reset
// record, index -1 --; otherwise the open version is shaded once more.
enum { AA_SUB_NONE = 0, AA_SUB_SAME = 1, AA_SUB_BEGIN = 2 };
MIRT_HD int aa_sub_event(AaRuns &runs, bool accepted, bool replaced)
{
    if (!accepted) return AA_SUB_NONE;
    if (replaced || runs.nver == 0) { runs.nver++; runs.count = 1; return AA_SUB_BEGIN; }
    runs.count++;
    return AA_SUB_SAME;
}

// The resolve's additions of one version: R = colour * (DirectLight + indirectLight) (:584-588) added `count` times, one at a time
// (:591).  `direct` is DirectLight's return value for the version's record, `tcol` the colour of the record's triangle.
MIRT_HD v3 aa_resolve_add(v3 avg, v3 tcol, v3 direct, v3 indirect, int count)
{
    const v3 R = mul3(tcol, add3(direct, indirect));
    for (int c = 0; c < count; c++) avg = add3(avg, R);
    return avg;
}
// pixelColours = avgColor / (realSamples * realSamples) (:599).
MIRT_HD v3 aa_resolve_div(v3 avg, int rs) { return div3s(avg, (float)(rs * rs)); }

}  // namespace mirt
