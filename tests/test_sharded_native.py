"""The native sharded entry points (mirt_band_of / mirt_band_plan / mirt_comm_* / mirt_*_sharded, csrc/comm.cpp).

Without a GPU: the band partition against mirt/sharding.py's, the gather plan applied to numpy buffers for 1..9 ranks and
ragged frames, and a C++ program that runs the plan with one process per rank (world sizes 2, 3, 5) over pipes.
-m gpu: two and three real processes on device 0 exchange their bands through the library's host-staged loopback transport
(MIRT_COMM=shm; RCCL needs one GPU per rank, which the driver's 8-GPU run provides) and the root's frames must equal
single-GPU frames byte for byte -- ray tracer (tile and binned kernels) and rasteriser, several frames per gather.  What one
GPU CAN run of the RCCL transport: a group of one rank -- the library is loaded (beside PyTorch's copy too), the communicator
created, a grouped ncclSend + ncclRecv to the rank itself compared byte for byte (mirt_comm_selfcheck), a sharded call made.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mirt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_band_of_matches_the_python_partition():
    from mirt.sharding import band_of
    for world in range(1, 10):
        for H in (0, 1, 7, 8, 9, 540, 1080, 4320, 4321):
            bands = [mirt.band_of(r, world, H) for r in range(world)]
            assert bands == [band_of(r, world, H) for r in range(world)]
            assert bands[0][0] == 0 and bands[-1][1] == H and all(a[1] == b[0] for a, b in zip(bands, bands[1:]))
    with pytest.raises(mirt.MirtError):
        mirt.band_of(3, 3, 100)


@pytest.mark.parametrize("world,root,W,H,nviews", [(1, 0, 5, 4, 2), (2, 0, 16, 9, 1), (2, 1, 7, 30, 3), (3, 1, 12, 10, 2), (8, 0, 6, 4321 // 100, 2), (9, 4, 3, 5, 1)])
def test_gather_plan_assembles_frames(world, root, W, H, nviews):
    """Applying the plan's byte moves to per-rank band buffers rebuilds every frame on the root."""
    rng = np.random.RandomState(world * 100 + H)
    full = rng.randint(0, 2 ** 32, (nviews, H, W), dtype=np.uint64).astype(np.uint32)
    bands = {}
    for r in range(world):
        y0, y1 = mirt.band_of(r, world, H)
        bands[r] = np.ascontiguousarray(full[:, y0:y1, :]).view(np.uint8).reshape(-1)
    frames = np.zeros((nviews, H, W), np.uint32)
    y0, y1 = mirt.band_of(root, world, H)
    frames[:, y0:y1] = full[:, y0:y1]
    flat = frames.view(np.uint8).reshape(-1)
    plan = mirt.band_plan(world, root, W, H, nviews)
    assert all(p[3] != root for p in plan)
    for ro, bo, nbytes, peer in plan:
        flat[ro:ro + nbytes] = bands[peer][bo:bo + nbytes]
    assert np.array_equal(frames, full)
    assert sum(p[2] for p in plan) == (H - (y1 - y0)) * W * 4 * nviews


@pytest.mark.parametrize("world,root,W,H,nviews,strip", [(2, 0, 16, 40, 1, 8), (3, 1, 7, 100, 2, 16), (8, 0, 6, 4320 // 10, 2, 64), (5, 4, 3, 9, 1, 8), (4, 2, 5, 64, 3, 64)])
def test_strip_partition_and_its_gather_plan(world, root, W, H, nviews, strip):
    """Interleaved strips: every row belongs to exactly one rank, strip s to rank s %% world, and the plan's byte moves rebuild every
    frame on the root from band buffers that hold each rank's strips of a view back to back."""
    owner = np.full(H, -1)
    for r in range(world):
        segs = mirt.partition_segments(r, world, H, strip)
        assert all(a % strip == 0 and (a // strip) % world == r and b == min(a + strip, H) for a, b in segs)
        for a, b in segs:
            assert (owner[a:b] == -1).all()
            owner[a:b] = r
    assert (owner >= 0).all()
    rng = np.random.RandomState(world * 1000 + H)
    full = rng.randint(0, 2 ** 32, (nviews, H, W), dtype=np.uint64).astype(np.uint32)
    bands = {r: np.concatenate([np.concatenate([full[v, a:b] for a, b in mirt.partition_segments(r, world, H, strip)] or [np.zeros((0, W), np.uint32)])
                                for v in range(nviews)]).view(np.uint8).reshape(-1) for r in range(world)}
    frames = np.zeros((nviews, H, W), np.uint32)
    for a, b in mirt.partition_segments(root, world, H, strip):
        frames[:, a:b] = full[:, a:b]
    flat = frames.view(np.uint8).reshape(-1)
    plan = mirt.partition_plan(world, root, W, H, nviews, strip)
    assert all(p[3] != root for p in plan)
    for ro, bo, nbytes, peer in plan:
        flat[ro:ro + nbytes] = bands[peer][bo:bo + nbytes]
    assert np.array_equal(frames, full)
    # strip_rows == 0 is the band partition
    assert mirt.partition_plan(world, root, W, H, nviews, 0) == mirt.band_plan(world, root, W, H, nviews)
    assert [s for r in range(world) for s in mirt.partition_segments(r, world, H, 0)] == [b for b in (mirt.band_of(r, world, H) for r in range(world)) if b[1] > b[0]]


def _weighted_bounds_reference(hist, shift, W, H, world, tile_weight=12):
    """csrc/comm.cpp: part_weighted_bounds, restated with Python integers (exact)."""
    tile_rows, tiles_x = (H + 7) // 8, (W + 7) // 8
    cost = []
    for j in range(tile_rows):
        c = j >> shift
        first, last = c << shift, min(tile_rows, (c + 1) << shift)
        h = int(hist[c]) if hist is not None and c < len(hist) else 0
        cost.append(h // max(last - first, 1) + tile_weight * tiles_x + 1)
    prefix = [0]
    for c in cost:
        prefix.append(prefix[-1] + c)
    total, bounds, j = prefix[-1], [0], 0
    for r in range(1, world):
        want = total * r
        while j < tile_rows and prefix[j + 1] * world <= want:
            j += 1
        cut = j
        if j < tile_rows and prefix[j + 1] * world - want < want - prefix[j] * world:
            cut = j + 1
        prev = (bounds[r - 1] + 7) // 8
        if tile_rows >= world:
            cut = min(max(cut, prev + 1), tile_rows - (world - r))
        cut = max(cut, prev)
        bounds.append(min(cut * 8, H))
    bounds.append(H)
    for r in range(1, world + 1):
        bounds[r] = max(bounds[r], bounds[r - 1])
    return bounds, cost


@pytest.mark.parametrize("H,W", [(4320, 7680), (1080, 1920), (131, 200), (64, 64), (9, 40), (0, 8)])
def test_weighted_bounds_split_the_estimated_cost_evenly(H, W):
    """mirt_weighted_bounds (MIRT_PARTITION_WEIGHTED): boundaries rise from 0 to H on tile rows, every rank keeps a tile row while
    there are enough, no band's cost is farther from the even share than one tile row's cost, and the result is the integer
    arithmetic of the restatement above -- what makes every rank of a group derive the same bands."""
    tile_rows = (H + 7) // 8
    shift = 0
    while ((max(tile_rows, 1) - 1) >> shift) + 1 > 256:
        shift += 1
    rows = ((max(tile_rows, 1) - 1) >> shift) + 1
    rng = np.random.RandomState(H + W)
    y = (np.arange(rows) + 0.5) / rows
    hists = {"none": None, "flat": np.full(rows, 100000, np.uint32), "zero": np.zeros(rows, np.uint32),
             "middle": (4e6 * np.exp(-((y - 0.5) / 0.2) ** 2)).astype(np.uint32), "top": (3e6 * (1 - y) ** 3).astype(np.uint32),
             "noise": rng.randint(0, 1 << 22, rows).astype(np.uint32), "one_row": (np.arange(rows) == rows // 3).astype(np.uint32) * np.uint32(4000000000)}
    for name, hist in hists.items():
        for world in (1, 2, 3, 4, 8, 9):
            got = mirt.weighted_bounds(hist, shift, W, H, world)
            want, cost = _weighted_bounds_reference(hist, shift, W, H, world)
            assert got == want, (name, world, got, want)
            assert got[0] == 0 and got[-1] == H and all(a <= b for a, b in zip(got, got[1:]))
            assert all(b % 8 == 0 or b == H for b in got)
            if tile_rows >= world:
                assert all(b > a for a, b in zip(got, got[1:])), (name, world, got)
            if H and name != "one_row":
                share = sum(cost) / world
                for a, b in zip(got, got[1:]):
                    band = sum(cost[a // 8:(b + 7) // 8])
                    assert abs(band - share) <= 2 * max(cost) + 1, (name, world, got, band, share)
    # equal costs give (nearly) equal bands; a peak in the middle makes the middle bands the shortest
    flat = mirt.weighted_bounds(hists["flat"], shift, W, H, 4)
    if tile_rows >= 8:
        sizes = [b - a for a, b in zip(flat, flat[1:])]
        assert max(sizes) - min(sizes) <= 16
        mid = mirt.weighted_bounds(hists["middle"], shift, W, H, 4)
        msizes = [b - a for a, b in zip(mid, mid[1:])]
        assert msizes[1] <= msizes[0] and msizes[2] <= msizes[3]


@pytest.mark.parametrize("world,root,W,H,nviews", [(2, 0, 16, 40, 1), (3, 1, 7, 100, 2), (8, 0, 6, 432, 2), (5, 4, 3, 9, 1), (4, 2, 5, 64, 3)])
def test_explicit_bounds_and_their_gather_plan(world, root, W, H, nviews):
    """Bands with explicit boundaries (what the weighted partition hands to the gather): the plan's byte moves rebuild every frame."""
    rng = np.random.RandomState(world * 77 + H)
    cuts = sorted(int(c) for c in rng.choice(np.arange(0, H + 1), world - 1))
    bounds = [0] + cuts + [H]
    full = rng.randint(0, 2 ** 32, (nviews, H, W), dtype=np.uint64).astype(np.uint32)
    bands = {r: np.ascontiguousarray(full[:, bounds[r]:bounds[r + 1], :]).view(np.uint8).reshape(-1) for r in range(world)}
    frames = np.zeros((nviews, H, W), np.uint32)
    frames[:, bounds[root]:bounds[root + 1]] = full[:, bounds[root]:bounds[root + 1]]
    flat = frames.view(np.uint8).reshape(-1)
    plan = mirt.bounds_plan(world, root, W, H, nviews, bounds)
    assert all(p[3] != root for p in plan)
    for ro, bo, nbytes, peer in plan:
        flat[ro:ro + nbytes] = bands[peer][bo:bo + nbytes]
    assert np.array_equal(frames, full)
    equal = [mirt.band_of(r, world, H)[0] for r in range(world)] + [H]
    assert mirt.bounds_plan(world, root, W, H, nviews, equal) == mirt.band_plan(world, root, W, H, nviews)
    with pytest.raises(mirt.MirtError):
        mirt.bounds_plan(world, root, W, H, nviews, [0] + [H + 8] * world)


@pytest.mark.parametrize("world,H", [(2, 40), (3, 100), (1, 9)])
def test_bounds_plan_rejects_boundaries_that_do_not_span_the_frame(world, H):
    """Boundaries that leave rows out at the top or the bottom are no partition of the frame: a plan built from them would gather a
    frame with rows nobody sends."""
    inner = [min(8 * r, H) for r in range(1, world)]
    plan = mirt.bounds_plan(world, 0, 16, H, 1, [0] + inner + [H])
    assert sum(p[2] for p in plan) == (H - inner[0] if inner else 0) * 16 * 4
    for bad in ([8] + inner + [H], [0] + inner + [H - 1], [1] + inner + [H - 1], [0] + inner + [max(inner + [0])]):
        with pytest.raises(mirt.MirtError):
            mirt.bounds_plan(world, 0, 16, H, 1, bad)


def test_cpp_world_size_2_partition_and_assembly(tmp_path):
    """tests/cpp/band_plan_test.cpp: one process per rank, bands through pipes in plan order, every word checked."""
    exe = str(tmp_path / "band_plan_test")
    csrc = os.path.join(ROOT, "cpp-raytracer-rasterizer_amd", "csrc")
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "band_plan_test.cpp"),
                    os.path.join(csrc, "comm.cpp"), "-o", exe, "-L/opt/rocm/lib", "-lamdhip64", "-ldl", "-lpthread", "-Wl,-rpath,/opt/rocm/lib"],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


RANK_CODE = r"""
import os, sys, numpy as np
sys.path[:0] = [%(pkg)r, %(tests)r]
import mirt
from devbuf import DeviceArray
rank, world, root = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
idfile = sys.argv[4]
mirt.init(rank if os.environ.get("MIRT_TEST_DEVICE_PER_RANK") == "1" else 0)
if rank == 0:
    cid = mirt.comm_create_id()
    with open(idfile + ".tmp", "wb") as f: f.write(cid)
    os.rename(idfile + ".tmp", idfile)
else:
    import time
    while not os.path.exists(idfile): time.sleep(0.01)
    cid = open(idfile, "rb").read()
mirt.comm_init(cid, rank, world)
strip = int(os.environ.get("MIRT_TEST_STRIP_ROWS", "0"))
mirt.set_partition(strip)
own = np.zeros(131, bool)
L = np.array([[0.0, -0.5, -0.7, 1, 1, 1, 14]], np.float32)
W, H = 200, 131
ok = True
# (the last one: a ray-traced batch right after a rasterised one of the same size -- the band buffers then hold rasterised
# pixels where the ray tracer writes nothing, the 1-pixel border, and those words must still travel as 0; then soft shadows of
# 3 x 16 = 48 light positions, set alike on every rank: each band is a deferred frame's, DirectLight in two passes)
L3 = np.array([[0.0, -0.5, -0.7, 1, 1, 1, 14], [0.5, 0.25, -0.875, 1, 0.5, 0.25, 6], [-0.375, 0.125, -0.625, 0.5, 1, 0.75, 9]], np.float32)
JIT = (np.repeat(L3[:, 0:3], 16, axis=0) + (np.random.default_rng(3).integers(-8, 9, (48, 3)) / 256.0)).astype(np.float32)
L1 = L
for kind, scene, soft in (("rt", "cornell", 0), ("rt", "soup", 0), ("raster", "cornell", 0), ("rt", "cornell", 0), ("rt", "cornell", 16)):
    L = L3 if soft else L1
    mirt.set_soft_shadows(soft or 1, JIT if soft else None)
    tris = mirt.scene_cornell() if scene == "cornell" else np.concatenate([mirt.scene_cornell(), mirt.scene_soup(4, 3000, 0.1)])
    views = [mirt.make_view((0.05 * i, 0, -2.6), mirt.rot_from_yaw(0.1 * i, 1.01 if kind == "raster" else 1.0), 70.0, W, H) for i in range(3)]
    mirt.scene_upload(tris, mirt.cull(tris, views[0], 0) if kind == "raster" else None)
    frames = DeviceArray((3, H, W), np.uint32, 0x33) if rank == root else None
    mode = mirt.RT_BINNED if scene == "soup" else mirt.RT_AUTO
    reps = 5 if strip < 0 else 3             # several gathers in a row: both band buffers, events; the weighted partition (strip -1)
    for rep in range(reps):                  # takes its bands from the histogram of the call before the previous one
        segs_root = [tuple(mirt.partition_bounds(world, W, H)[root:root + 2])] if strip < 0 else mirt.partition_segments(root, world, H, strip)
        mirt.prepared_sharded(kind, views, L, (0.2, 0.2, 0.2), mode, root, frames.ptr if frames else None, W * 4)()
    if strip < 0 and scene == "soup" and world > 1:
        # the soup is binned, so by now the bands come from a histogram: not the equal split any more (3 000 triangles around the
        # box crowd the middle rows)
        used = mirt.partition_bounds(world, W, H)
        assert used != [mirt.band_of(r, world, H)[0] for r in range(world)] + [H], used
    mirt.sync()
    if rank == root:
        got = frames.read()
        for i, v in enumerate(views):
            ref = DeviceArray((H, W), np.uint32, 0x33)
            if kind == "rt":
                mirt.raytrace_device(v, L, (0.2, 0.2, 0.2), mode, 0, H, 0, ref.ptr, W * 4)
            else:
                mirt.rasterise_device(v, L, (0.2, 0.2, 0.2), 0, H, 0, ref.ptr, W * 4)
            want = ref.read()
            if kind == "rt":
                # border words: the ray tracer never writes them -- the root's own rows keep the caller's fill, received bands carry 0
                border = np.zeros((H, W), bool)
                border[0, :] = border[-1, :] = True; border[:, 0] = border[:, -1] = True
                own = np.zeros((H, W), bool)
                for ry0, ry1 in segs_root:
                    own[ry0:ry1] = True
                want[border & own] = 0x33333333
                want[border & ~own] = 0
            if not np.array_equal(got[i], want):
                ok = False
                print("MISMATCH", kind, scene, "soft", soft, "view", i, int((got[i] != want).sum()), flush=True)
            assert (got[i][1:-1, 1:-1] != 0x33333333).any()
mirt.comm_shutdown()
mirt.shutdown()
print("rank %%d done ok=%%s" %% (rank, ok), flush=True)
sys.exit(0 if ok else 1)
"""


@pytest.mark.gpu
@pytest.mark.parametrize("world,root,strip", [(2, 0, 0), (3, 1, 0), (2, 1, 16), (3, 0, 8), (2, 0, -1), (3, 1, -1)])
def test_sharded_frames_through_the_loopback_transport(tmp_path, world, root, strip):
    code = RANK_CODE % {"pkg": os.path.join(ROOT, "cpp-raytracer-rasterizer_amd"), "tests": os.path.join(ROOT, "tests")}
    env = dict(os.environ, MIRT_COMM="shm", MIRT_TEST_STRIP_ROWS=str(strip))
    idfile = str(tmp_path / "comm_id")
    procs = [subprocess.Popen([sys.executable, "-c", code, str(r), str(world), str(root), idfile], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)


AGREE_CODE = r"""
import json, os, sys, time, numpy as np
sys.path[:0] = [%(pkg)r, %(tests)r]
import mirt
from devbuf import DeviceArray
rank, world, root, idfile, logdir, seq = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5], sys.argv[6]
mirt.init(rank if os.environ.get("MIRT_TEST_DEVICE_PER_RANK") == "1" else 0)
if rank == 0:
    cid = mirt.comm_create_id()
    with open(idfile + ".tmp", "wb") as f: f.write(cid)
    os.rename(idfile + ".tmp", idfile)
else:
    while not os.path.exists(idfile): time.sleep(0.01)
    cid = open(idfile, "rb").read()
mirt.comm_init(cid, rank, world)
mirt.set_frames_in_flight(1)
mirt.set_partition(mirt.PARTITION_WEIGHTED)
L = np.array([[0.0, -0.5, -0.7, 1, 1, 1, 14]], np.float32)
IND = (0.2, 0.2, 0.2)
# about 2 000 triangles packed in a horizontal slab above the middle of the frame: most of the cost lies in a few tile rows near
# the top, so the weighted bands there are thin and the bottom one is tall
tris = mirt.scene_soup(7, 2000, 0.06)
for k in (1, 4, 7):
    tris[:, k] = tris[:, k] * np.float32(0.08) - np.float32(0.45)
W, H = (160 if world == 2 else 320), 240      # (two ranks: a narrow frame, whose MIRT_RT_AUTO threshold -- 125 rows -- the top band stays below)
nviews, mode, ncalls = 1, mirt.RT_AUTO, 12
if seq == "b":
    nviews, mode = 2, mirt.RT_BINNED
elif seq == "c":
    mode = mirt.RT_BINNED
    if os.environ.get("MIRT_TEST_HIST") == "1" and rank == 0:
        mirt.set_cost_histogram(1)
elif seq == "d":
    mode, H, ncalls = mirt.RT_BINNED, 8 * (world - 1) - 1, 10    # fewer tile rows than ranks: some band is empty
mirt.scene_upload(tris)
def view(i):
    # the camera moves every call: sideways, turning, and up and down so that the slab (and with it the cost) moves between rows
    return mirt.make_view((0.03 * i, 0.35 * np.sin(0.7 * i), -2.6), mirt.rot_from_yaw(0.02 * i, 1.0), 200.0, W, H)
def kind_of(c):
    return "raster" if seq == "d" and c == 5 else "rt"
def check_agreement(c, bounds):
    with open(os.path.join(logdir, "c%%d_r%%d.tmp" %% (c, rank)), "w") as f: json.dump(bounds, f)
    os.rename(os.path.join(logdir, "c%%d_r%%d.tmp" %% (c, rank)), os.path.join(logdir, "c%%d_r%%d.json" %% (c, rank)))
    deadline, table = time.time() + 60.0, {}
    while len(table) < world:
        for r in range(world):
            p = os.path.join(logdir, "c%%d_r%%d.json" %% (c, r))
            if r not in table and os.path.exists(p):
                table[r] = json.load(open(p))
        if len(table) < world:
            if time.time() > deadline:
                print("rank %%d: call %%d: no bounds from ranks %%s within 60 s" %% (rank, c, sorted(set(range(world)) - set(table))), flush=True)
                os._exit(4)
            time.sleep(0.005)
    if any(table[r] != table[0] for r in range(world)):
        # a plan the ranks disagree on must never reach the gather: the grouped send / receive would wait forever
        print("rank %%d: call %%d (%%s, seq %%s): the ranks derived different bounds:" %% (rank, c, kind_of(c), seq), flush=True)
        for r in range(world):
            print("  rank %%d: %%s" %% (r, table[r]), flush=True)
        os._exit(3)
frames, calls = [], []
for c in range(ncalls):
    views = [view(c + k) for k in range(nviews)]              # (seq b: view 1 of call c is view 0 of call c + 1)
    bounds = mirt.partition_bounds(world, W, H)
    check_agreement(c, bounds)
    kind = kind_of(c)
    buf = DeviceArray((nviews, H, W), np.uint32, 0x33) if rank == root else None
    mirt.prepared_sharded(kind, views, L, IND, mode, root, buf.ptr if buf else None, W * 4)()
    frames.append(buf)
    calls.append((kind, views, bounds))
    if seq == "c" and rank == 0 and c in (3, 6):
        # frames outside sharded calls, on rank 0 alone: one, later five in a row (binned, whole frames, views of their own)
        with DeviceArray((H, W), np.uint32) as own:
            for k in range(1 if c == 3 else 5):
                mirt.raytrace_device(view(40 + 3 * k + c), L, IND, mirt.RT_BINNED, 0, H, 0, own.ptr, W * 4)
            mirt.sync()
mirt.sync()
ok = True
if rank == root:
    for c, ((kind, views, bounds), buf) in enumerate(zip(calls, frames)):
        got = buf.read()
        for i, v in enumerate(views):
            with DeviceArray((H, W), np.uint32, 0x33) as ref:
                if kind == "rt":
                    mirt.raytrace_device(v, L, IND, mode, 0, H, 0, ref.ptr, W * 4)
                else:
                    mirt.rasterise_device(v, L, IND, 0, H, 0, ref.ptr, W * 4)
                want = ref.read()
            if kind == "rt":
                # border words: the ray tracer never writes them -- the root's own rows keep the caller's fill, received bands carry 0
                border = np.zeros((H, W), bool)
                border[0, :] = border[-1, :] = True; border[:, 0] = border[:, -1] = True
                own = np.zeros((H, W), bool)
                own[bounds[root]:bounds[root + 1]] = True
                want[border & own] = 0x33333333
                want[border & ~own] = 0
            if not np.array_equal(got[i], want):
                ok = False
                print("MISMATCH call", c, kind, "view", i, int((got[i] != want).sum()), "bounds", bounds, flush=True)
        buf.free()
mirt.comm_shutdown()
mirt.shutdown()
print("rank %%d done ok=%%s" %% (rank, ok), flush=True)
sys.exit(0 if ok else 1)
"""


def _run_ranks(code, world, args, env, timeout=600):
    procs = [subprocess.Popen([sys.executable, "-c", code, str(r), str(world)] + list(args), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)


def _logged_bounds(logdir, world):
    """The bounds every call used, as the ranks logged them before the call (they agree, or the run has failed already)."""
    calls = []
    while os.path.exists(os.path.join(logdir, "c%d_r0.json" % len(calls))):
        calls.append(json.load(open(os.path.join(logdir, "c%d_r0.json" % len(calls)))))
    return calls


def _auto_bins(rows, W, n=2000):
    """capi/rt_frame.cpp: the rows of a band that MIRT_RT_AUTO bins (what decides whether a band's pass files anything)."""
    return n >= 65 and W * rows > 4096 and W * rows * n >= 40000000


def _assert_trigger(seq, world, calls):
    """That the situation each sequence is about really arose -- decided from the logged bounds (the inputs of every rank's
    choice), not from what the library did with them."""
    bands = [[b[r + 1] - b[r] for r in range(world)] for b in calls]
    equal = [mirt.band_of(r, world, 240)[0] for r in range(world)] + [240]
    if seq == "a":
        # in some call, one rank's band is binned by MIRT_RT_AUTO and another's is rendered brute force (AGREE_CODE's frame width)
        W = 160 if world == 2 else 320
        assert any(len({_auto_bins(rows, W) for rows in rs}) == 2 for rs in bands), calls
    elif seq == "b":
        # in some call, one rank's band is the one it had in the call before (its pass of view 0 can be kept) and another's moved
        assert any(any(a[r:r + 2] == b[r:r + 2] for r in range(world)) and any(a[r:r + 2] != b[r:r + 2] for r in range(world))
                   for a, b in zip(calls, calls[1:])), calls
    elif seq == "c":
        # the calls after rank 0's frames of its own used cost-weighted bands
        assert all(b != equal for b in calls[8:]), calls
    elif seq == "d":
        # some rank's band is empty
        assert any(0 in rs for rs in bands), calls


@pytest.mark.gpu
@pytest.mark.parametrize("seq,world,root,hist", [("a", 2, 0, 0), ("a", 3, 2, 0), ("b", 3, 0, 0), ("b", 3, 1, 0),
                                                  ("c", 2, 1, 0), ("c", 3, 0, 1), ("c", 2, 0, 1), ("d", 2, 1, 0), ("d", 3, 0, 0)])
def test_ranks_derive_the_same_weighted_bounds_on_every_call(tmp_path, seq, world, root, hist):
    """MIRT_PARTITION_WEIGHTED: every rank derives the band boundaries of every sharded call from its own copy of the cost
    histogram, nothing exchanged.  Before each call every rank logs mirt_partition_bounds and waits for the
    others'; ranks that disagree stop there, before a plan they disagree on can reach the gather.  The sequences are the ways a
    rank's own history could make it file other histograms than its peers: (a) MIRT_RT_AUTO with bands on both sides of the
    binning threshold; (b) two views per call, the second the next call's first, so that a rank whose band did not move could keep
    its pass of view 0; (c) frames rank 0 alone renders between sharded calls, with and without mirt_set_cost_histogram(1); (d) a
    frame shorter than 8 rows per rank (empty bands) and a rasterised call in the ray-traced sequence.  Each asserts that its
    situation arose; the root's frames must equal single-GPU frames.  (Sequence (b) needs three ranks: with two, both bands move
    whenever the one boundary does.)"""
    code = AGREE_CODE % {"pkg": os.path.join(ROOT, "cpp-raytracer-rasterizer_amd"), "tests": os.path.join(ROOT, "tests")}
    env = dict(os.environ, MIRT_COMM="shm", MIRT_TEST_HIST=str(hist))
    logdir = tmp_path / "bounds"
    logdir.mkdir()
    _run_ranks(code, world, [str(root), str(tmp_path / "comm_id"), str(logdir), seq], env)
    _assert_trigger(seq, world, _logged_bounds(str(logdir), world))


SELF_CODE = r"""
import os, sys, numpy as np
sys.path[:0] = [%(pkg)r, %(tests)r]
dist = None
if sys.argv[1] == "torch":
    # as in bench.py --gpus N: the process runs torch.distributed over RCCL (its own communicator, made by an all_reduce)
    # before AND after the library creates its group -- two users of RCCL in one process
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%%d" %% (20000 + os.getpid() %% 20000), rank=0, world_size=1)
    t = torch.ones(4, device="cuda:0")
    dist.all_reduce(t)
    assert t.sum().item() == 4.0
    ids = [None]
    dist.broadcast_object_list(ids, src=0)    # how bench.py hands the group id to the ranks
import mirt
from devbuf import DeviceArray
mirt.init(0)
mirt.comm_init(mirt.comm_create_id(), 0, 1)
for nbytes in (1, 4096, 8 << 20):
    mirt.comm_selfcheck(nbytes)
tris = mirt.scene_cornell()
mirt.scene_upload(tris)
W, H = 160, 90
views = [mirt.make_view((0.05 * i, 0, -2.6), mirt.rot_from_yaw(0.1 * i, 1.0), 70.0, W, H) for i in range(2)]
L = np.array([[0.0, -0.5, -0.7, 1, 1, 1, 14]], np.float32)
frames = DeviceArray((2, H, W), np.uint32, 0x33)
mirt.set_frames_in_flight(1)
mirt.prepared_sharded("rt", views, L, (0.2, 0.2, 0.2), mirt.RT_AUTO, 0, frames.ptr, W * 4)()
mirt.sync()
got = frames.read()
for i, v in enumerate(views):
    ref = DeviceArray((H, W), np.uint32, 0x33)
    mirt.raytrace_device(v, L, (0.2, 0.2, 0.2), mirt.RT_AUTO, 0, H, 0, ref.ptr, W * 4)
    assert np.array_equal(got[i], ref.read())
if dist is not None:
    t = torch.ones(4, device="cuda:0")
    dist.all_reduce(t)
    torch.cuda.synchronize()
    assert t.sum().item() == 4.0
mirt.comm_shutdown()
mirt.shutdown()
if dist is not None:
    dist.destroy_process_group()
print("selfcheck ok", flush=True)
"""


@pytest.mark.gpu
@pytest.mark.parametrize("strip", [0, -1])
def test_sharded_frames_over_rccl_on_two_devices(tmp_path, strip):
    """The same frames with one rank per DEVICE and the library's RCCL transport (grouped ncclSend / ncclRecv over xGMI): the
    multi-GPU path as bench.py --gpus N runs it.  Needs two GPUs; skipped on a one-GPU box (where the loopback transport and the
    group of one rank above are what can run)."""
    import torch
    if torch.cuda.device_count() < 2:                  # (counting devices does not initialise the GPU in this process)
        pytest.skip("needs two GPUs")
    code = RANK_CODE % {"pkg": os.path.join(ROOT, "cpp-raytracer-rasterizer_amd"), "tests": os.path.join(ROOT, "tests")}
    env = {k: v for k, v in os.environ.items() if k != "MIRT_COMM"}
    env["MIRT_TEST_DEVICE_PER_RANK"] = "1"
    env["MIRT_TEST_STRIP_ROWS"] = str(strip)               # 0: equal bands, -1: the cost-weighted partition
    idfile = str(tmp_path / "comm_id")
    procs = [subprocess.Popen([sys.executable, "-c", code, str(r), "2", "0", idfile], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    if strip == -1:
        # and every rank derives the same weighted bounds on every call over RCCL too (the sequences of the loopback test above)
        code = AGREE_CODE % {"pkg": os.path.join(ROOT, "cpp-raytracer-rasterizer_amd"), "tests": os.path.join(ROOT, "tests")}
        for seq in ("a", "c", "d"):
            logdir = tmp_path / ("bounds_" + seq)
            logdir.mkdir()
            _run_ranks(code, 2, ["0", str(tmp_path / ("comm_id_" + seq)), str(logdir), seq], dict(env, MIRT_TEST_HIST="1"))
            _assert_trigger(seq, 2, _logged_bounds(str(logdir), 2))


@pytest.mark.gpu
@pytest.mark.parametrize("host", ["plain", "torch"])
def test_rccl_group_of_one_rank(host):
    code = SELF_CODE % {"pkg": os.path.join(ROOT, "cpp-raytracer-rasterizer_amd"), "tests": os.path.join(ROOT, "tests")}
    env = {k: v for k, v in os.environ.items() if k != "MIRT_COMM"}
    r = subprocess.run([sys.executable, "-c", code, host], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "selfcheck ok" in r.stdout, r.stdout + r.stderr
