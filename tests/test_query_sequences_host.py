"""What the sequences of tests/fuzz_queries.py contain, checked on the CPU for exactly the seeds tests/test_gpu_query_sequences.py runs:
generate() and a dry pass of the Model with the oracle, no device.  A green run on the GPU only means something when the inputs
reach what they are meant to reach -- every op kind often enough, the ordered pairs of calls between which a stale key, a missing
wait or a shared scratch buffer would show, and oracle answers that are neither all hits nor all misses.  Every failure message
carries the counts that were achieved."""
import collections
import json

import pytest

import mirt
import fuzz_queries as fq

FIRST, COUNT = fq.SUITE_SEEDS
FAN_OPS = ("intersect_fans", "occluded_fans")
CAN_BIN = ("intersect_from", "intersect_fans", "occluded_fans", "direct_light")       # (intersect and occluded always sweep)


@pytest.fixture(scope="module")
def sequences(oracle):
    """[(seed, ops, plans)]: computed once, shared, never changed."""
    out = []
    for seed in range(FIRST, FIRST + COUNT):
        ops = fq.generate(seed)
        out.append((seed, ops, fq.Model(oracle).run(ops)))
    return out


def kind_of(op):
    name = op["op"]
    return name[:-7] if name.endswith("_device") else name


def no_scene_op(ops, i, j):
    return not any(o["op"] in fq.SCENE_OPS for o in ops[i + 1:j])


def test_generate_is_deterministic_and_plain():
    for seed in range(FIRST, FIRST + COUNT):
        ops = fq.generate(seed)
        assert ops == fq.generate(seed)
        assert 25 <= len(ops) <= 40, (seed, len(ops))
        assert ops[-1] == {"op": "sync"}
        for op in ops:
            assert op["op"] in fq.OP_KINDS
            for v in op.values():
                assert isinstance(v, (int, float, str)) or (isinstance(v, list) and len(v) <= 8 and all(
                    isinstance(x, (int, float)) or (isinstance(x, list) and len(x) <= 4 and all(isinstance(y, (int, float)) for y in x)) for x in v)), op
            assert json.loads(json.dumps(op)) == op


def test_every_op_kind_form_and_mode_occurs(sequences):
    count = collections.Counter(op["op"] for _, ops, _ in sequences for op in ops)
    assert all(count[k] >= 5 for k in fq.OP_KINDS), sorted(count.items())
    combos = collections.Counter((p["kind"], p["device"], p["qmode"]) for _, ops, plans in sequences for op, p in zip(ops, plans) if op["op"] in fq.QUERY_OPS)
    missing = [(k, d, m) for k in fq.QUERY_KINDS for d in (False, True) for m in (mirt.QUERY_AUTO, mirt.QUERY_BRUTE, mirt.QUERY_BINNED) if not combos[(k, d, m)]]
    assert not missing, (missing, sorted(combos.items()))
    frames = collections.Counter((op["op"], p["W"], p["deferred"]) for _, ops, plans in sequences for op, p in zip(ops, plans) if op["op"] in fq.FRAME_OPS)
    assert sum(v for k, v in frames.items() if k[2]) >= 5 and sum(v for k, v in frames.items() if k[1] == 72) >= 5, sorted(frames.items())
    extras = collections.Counter()
    for _, ops, plans in sequences:
        for op, p in zip(ops, plans):
            for flag in ("odd", "carried", "repeat", "check", "bands", "planes"):
                extras[flag] += bool(op.get(flag))
            extras["limits None"] += op.get("limits") == 0
            extras["origins == positions"] += op.get("origins") == "positions"
            extras["K %s" % op.get("origins")] += op["op"].startswith(FAN_OPS)
            extras["no origin_of"] += op["op"].startswith(FAN_OPS) and not op["origin_of"]
            extras["snapshot"] += bool(op.get("snapshot"))
    want = ["odd", "carried", "repeat", "check", "bands", "planes", "limits None", "origins == positions", "K 1", "K 3", "K 32", "K 33", "no origin_of", "snapshot"]
    assert all(extras[k] >= 2 for k in want), sorted(extras.items())


def pairs_of(ops, plans):
    """The ordered pairs of the module docstring found in one sequence, as a Counter of their names."""
    found = collections.Counter()
    n = len(ops)
    for i in range(n):
        a, pa = ops[i], plans[i]
        ka = kind_of(a)
        later = [(j, ops[j], plans[j], kind_of(ops[j])) for j in range(i + 1, n)]
        if a["op"] in ("scene_update", "scene_update_device", "scene_transform", "scene_pose"):
            seen = set()                                                 # the first query of each kind after the scene op
            for j, b, pb, kb in later:
                if b["op"] in fq.SCENE_OPS:
                    break
                if kb in fq.QUERY_KINDS and kb not in seen:
                    seen.add(kb)
                    if kb not in CAN_BIN or pb["qmode"] == mirt.QUERY_BINNED:
                        found["%s -> %s" % (ka, kb)] += 1
        if ka == "direct_light":
            for j, b, pb, kb in later:
                if b["op"] in fq.SCENE_OPS:
                    break
                if kb in FAN_OPS and pa["qmode"] == mirt.QUERY_BINNED and pa["npos"] <= 32 and pb["qmode"] == mirt.QUERY_BINNED and pb["origins"] == pa["positions"]:
                    found["direct_light (binned, <= 32) -> fans on its positions"] += 1
                    break
            for j, b, pb, kb in later:
                if b["op"] in fq.SCENE_OPS:
                    break
                if kb == "direct_light":
                    if pa["npos"] >= 33 and pb["npos"] >= 33 and pb["positions"] != pa["positions"]:
                        found["direct_light (>= 33) -> direct_light (other >= 33)"] += 1
                    break
        if a["op"] in ("raytrace", "raytrace_device", "raytrace_sharded") and a["mode"] == mirt.RT_BINNED and pa["nscene"] >= 65 and pa["npos"] <= 32:
            for j, b, pb, kb in later:
                if b["op"] in fq.SCENE_OPS or b["op"] in fq.FRAME_OPS:
                    break
                if kb == "intersect_fans" and pb["origins"] == pa["positions"]:
                    found["binned frame -> intersect_fans on its lights"] += 1
                    break
        if a["op"] == "raytrace_device" and pa["deferred"] and pa["flight"] >= 2:
            for j, b, pb, kb in later:
                if b["op"] in fq.SCENE_OPS or b["op"] == "sync":
                    break
                if b["op"] == "direct_light_device" and pb["npos"] >= 33 and pb["positions"] != pa["positions"]:
                    found["deferred frame in flight -> direct_light_device (other >= 33)"] += 1
                    break
        if ka.startswith("intersect"):
            moved = False
            for j, b, pb, kb in later:
                if kb.startswith("intersect"):
                    break
                moved = moved or b["op"] in fq.SCENE_OPS and b["op"] != "scene_set_objects"
                if kb == "direct_light":
                    found["intersect -> scene op -> direct_light on the carried records"] += moved
                    break
        if ka.startswith("occluded"):
            for j, b, pb, kb in later:
                if b["op"] in fq.SCENE_OPS or kb in fq.QUERY_KINDS:
                    break
                if b["op"] in ("query_stats", "fan_stats"):
                    found["occluded* -> query_stats / fan_stats"] += 1
                    break
        if a["op"] == "rasterise" and not a["device"]:
            for j, b, pb, kb in later:
                if b["op"] in fq.SCENE_OPS:
                    break
                if b["op"] == "raytrace" and pb["W"] * pb["H"] > pa["W"] * pa["H"]:
                    found["rasterise -> larger raytrace with want_intersection"] += 1
                    break
    return found


def test_ordered_pairs_occur(sequences):
    found = collections.Counter()
    for _, ops, plans in sequences:
        found.update(pairs_of(ops, plans))
    want = ["%s -> %s" % (s, q) for s in fq.MOVING_OPS for q in fq.QUERY_KINDS]
    want += ["direct_light (binned, <= 32) -> fans on its positions", "binned frame -> intersect_fans on its lights",
             "direct_light (>= 33) -> direct_light (other >= 33)", "deferred frame in flight -> direct_light_device (other >= 33)",
             "intersect -> scene op -> direct_light on the carried records", "occluded* -> query_stats / fan_stats",
             "rasterise -> larger raytrace with want_intersection"]
    short = [k for k in want if found[k] < 2]
    assert not short, (short, sorted(found.items()))


def test_oracle_answers_are_of_both_kinds(sequences):
    rates, frames, bad = [], [], []
    for seed, ops, plans in sequences:
        for i, (op, p) in enumerate(zip(ops, plans)):
            if "rate" in p:
                rates.append(p["rate"])
                if not 0.10 <= p["rate"] <= 0.90:
                    bad.append((seed, i, op, p["rate"]))
            if "hit" in p:
                frames.append(min(p["hit"], p["missed"]))
                if p["hit"] < 50 or p["missed"] < 50:
                    bad.append((seed, i, op, p["hit"], p["missed"]))
    assert rates and frames
    assert not bad, (bad, "rates %.2f .. %.2f over %d batches; fewest pixels of a kind %d over %d frames" % (min(rates), max(rates), len(rates), min(frames), len(frames)))


def summary(sequences):
    """The achieved counts, as SUMMARY reports them (python -c 'import ...; print(summary(...))')."""
    found, count = collections.Counter(), collections.Counter()
    for _, ops, plans in sequences:
        found.update(pairs_of(ops, plans))
        count.update(op["op"] for op in ops)
    return dict(ops=dict(count), pairs=dict(found))
