"""Scenes placed away from the world origin: what test_along_host.py, test_gpu_placement.py and the placed probe cases share.

A placement (offset T, scale s) maps x to x * s + T, in float64, rounded once to float32 (place).  It is applied alike to triangle
vertices (normals and colours kept), cameras, light positions, fan origins, ray starts and record positions; directions are only
scaled, and a light's power takes s^2, so that in exact arithmetic the placed call is the unit call.  The oracle always runs on the
placed float32 values: nothing here compares a placed result with a unit one.

A pure scaling multiplies every operand of a binning margin alike; an offset does not -- the scene's extent R = max |coordinate|, the
reach smax = 8 R and the grid's corner |p0| grow with |T| while the cells keep the scene's size.  ALONG_CLASS says what that does to
the grid across a direction (along/along.hpp): its every-ray list grows (`binned`, still), then outgrows along_every_cap (`gave_up`),
then the cells are finer than a float resolves at that distance and no descriptor is made (`no_grid`).  The table is derived from the
header by tests/cpp/along_bins_test.cpp's scene-file mode, which test_along_host.py runs again on every entry.

The arbitrary-ray grid (grid/ray_grid.hpp) meets an offset sooner: its plane index grows with the scene's distance from the origin
over its triangles' size, then the every-ray list outgrows grid_every_cap.  RAY_GRID says, per scene and placement of GRID_PLACEMENTS
-- PLACEMENTS and GRID_EDGE, the last step along (10, -7, 5) at which soup2000 still bins --, the class and the counts
tests/cpp/ray_grid_test.cpp's scene-file mode reports (test_ray_grid_host.py runs it again on every entry).  TIE_SCENE is soup2000
with its first rows twice: equal distances with two indices in every placement (test_gpu_placement_grid.py, placed_grid.py)."""
import numpy as np

import mirt
from along_helpers import OBLIQUE

# name -> (offset T, scale s)
PLACEMENTS = {
    "unit": ((0.0, 0.0, 0.0), 1.0),
    "3_0_0": ((3.0, 0.0, 0.0), 1.0),                               # the box straddles binades: [2, 4] in x
    "10_-7_5": ((10.0, -7.0, 5.0), 1.0),
    "300_200_-100": ((300.0, 200.0, -100.0), 1.0),                 # a level in game units, a CAD part in millimetres
    "1000_1000_1000": ((1000.0, 1000.0, 1000.0), 1.0),
    "origin_x1024": ((0.0, 0.0, 0.0), 2.0 ** 10),
    "origin_div1024": ((0.0, 0.0, 0.0), 2.0 ** -10),
    "40_-25_60_div1024": ((40.0, -25.0, 60.0), 2.0 ** -10),
    "10_-7_5_div1024": ((10.0, -7.0, 5.0), 2.0 ** -10),
    "0_0_4096": ((0.0, 0.0, 4096.0), 1.0),
}
FAR = "300_200_-100"
# the last step along (10, -7, 5) at which the arbitrary-ray grid still bins soup2000 (RAY_GRID_CLASS): the ray grid's tests alone visit it
GRID_EDGE = "20_-14_10"
GRID_PLACEMENTS = dict(PLACEMENTS, **{GRID_EDGE: ((20.0, -14.0, 10.0), 1.0)})
# the tie scene: soup2000 followed by a copy of its first TIE_ROWS rows -- placed duplicates stay exact duplicates, so equal distances
# with two indices survive every placement (2100 triangles: the ray grid has 32 cells a side, the along grids 64)
TIE_SCENE, TIE_ROWS = "soup2000+dup", 100

# the directions of the along / alongs calls, before scaling: the oblique one, an axis, and three more for the call of five
ALONG_DIRS = {"oblique": OBLIQUE, "-y": np.array([0, -1, 0], np.float32), "+x": np.array([1, 0, 0], np.float32),
              "xy": np.array([1, 1, 0], np.float32), "slant": np.array([-0.9, 0.05, 0.3], np.float32)}
SINGLE_DIRS = ("oblique", "-y")

_scenes = {}


def place(x, T, s):
    """x * s + T in float64, rounded once to float32; x: (..., 3)."""
    return (np.asarray(x, np.float64) * float(s) + np.asarray(T, np.float64)).astype(np.float32)


def place_dirs(d, s):
    """Directions are scaled only."""
    return (np.asarray(d, np.float64) * float(s)).astype(np.float32)


def place_tris(tris, T, s):
    """Rows of 15 floats with their nine vertex coordinates placed; normals and colours kept."""
    out = np.array(tris, np.float32).reshape(-1, 15)
    out[:, 0:9] = place(out[:, 0:9].reshape(-1, 3, 3), T, s).reshape(-1, 9)
    return out


def place_lights(lights7, T, s):
    """Rows {position, colour, power}: the position placed, the power times s^2 (DirectLight divides by 4 pi r^2)."""
    out = np.array(lights7, np.float32).reshape(-1, 7)
    out[:, 0:3] = place(out[:, 0:3], T, s)
    out[:, 6] = (out[:, 6].astype(np.float64) * float(s) ** 2).astype(np.float32)
    return out


def unit_scene(name):
    """The suite's scenes by name, as they are at the origin (computed once, read-only)."""
    if name not in _scenes:
        if name == "soup2000":
            v = mirt.scene_soup(41, 2000, 0.2)
        elif name == "cornell+soup2000":
            v = np.concatenate([mirt.scene_cornell(), mirt.scene_soup(41, 2000, 0.2)])
        elif name == TIE_SCENE:
            v = np.concatenate([unit_scene("soup2000"), unit_scene("soup2000")[:TIE_ROWS]])
        elif name == "soup33000":
            v = mirt.scene_soup(77, 33000, 0.05)
        else:
            raise KeyError(name)
        v.setflags(write=False)
        _scenes[name] = v
    return _scenes[name]


def placed_scene(name, pname):
    key = (name, pname)
    if key not in _scenes:
        v = place_tris(unit_scene(name), *GRID_PLACEMENTS[pname])
        v.setflags(write=False)
        _scenes[key] = v
    return _scenes[key]


def extent_of(tris):
    """R: the largest |coordinate| of the scene's vertices."""
    return float(np.abs(np.asarray(tris).reshape(-1, 15)[:, :9]).max())


def alongs_class(scene, pname):
    """The class of a call of all five directions: one that has no grid, or gave up, takes the whole call to the brute-force kernels."""
    classes = [ALONG_CLASS[scene][pname][k] for k in range(len(ALONG_DIRS))]
    return "no_grid" if "no_grid" in classes else "gave_up" if "gave_up" in classes else "binned"


def along_class(scene, pname, dname):
    return ALONG_CLASS[scene][pname][list(ALONG_DIRS).index(dname)]


# scene -> placement -> the class per direction of ALONG_DIRS, in its order (every-ray counts: test_along_host.py prints them)
ALONG_CLASS = {
    "soup2000": {
        "unit": ("binned", "binned", "binned", "binned", "binned"),
        "3_0_0": ("binned", "binned", "binned", "binned", "binned"),
        "10_-7_5": ("binned", "binned", "binned", "binned", "binned"),
        "300_200_-100": ("binned", "binned", "binned", "binned", "binned"),
        "1000_1000_1000": ("binned", "gave_up", "gave_up", "binned", "gave_up"),
        "origin_x1024": ("binned", "binned", "binned", "binned", "binned"),
        "origin_div1024": ("binned", "binned", "binned", "binned", "binned"),
        "40_-25_60_div1024": ("gave_up", "no_grid", "no_grid", "no_grid", "no_grid"),
        "10_-7_5_div1024": ("no_grid", "no_grid", "no_grid", "no_grid", "no_grid"),
        "0_0_4096": ("no_grid", "no_grid", "no_grid", "no_grid", "no_grid"),
    },
    "cornell+soup2000": {
        "unit": ("binned", "binned", "binned", "binned", "binned"),
        "3_0_0": ("binned", "binned", "binned", "binned", "binned"),
        "10_-7_5": ("binned", "binned", "binned", "binned", "binned"),
        "300_200_-100": ("binned", "binned", "binned", "binned", "binned"),
        "1000_1000_1000": ("binned", "gave_up", "gave_up", "binned", "gave_up"),
        "origin_x1024": ("binned", "binned", "binned", "binned", "binned"),
        "origin_div1024": ("binned", "binned", "binned", "binned", "binned"),
        "40_-25_60_div1024": ("gave_up", "no_grid", "no_grid", "no_grid", "no_grid"),
        "10_-7_5_div1024": ("no_grid", "no_grid", "no_grid", "no_grid", "no_grid"),
        "0_0_4096": ("no_grid", "no_grid", "no_grid", "no_grid", "no_grid"),
    },
    "soup33000": {                                                  # B = 256: eight times finer cells, refused eight times sooner
        "unit": ("binned", "binned", "binned", "binned", "binned"),
        "3_0_0": ("binned", "binned", "binned", "binned", "binned"),
        "10_-7_5": ("binned", "binned", "binned", "binned", "binned"),
        "300_200_-100": ("binned", "no_grid", "no_grid", "no_grid", "no_grid"),
        "1000_1000_1000": ("no_grid", "no_grid", "no_grid", "no_grid", "no_grid"),
        "origin_x1024": ("binned", "binned", "binned", "binned", "binned"),
        "origin_div1024": ("binned", "binned", "binned", "binned", "binned"),
        "40_-25_60_div1024": ("no_grid", "no_grid", "no_grid", "no_grid", "no_grid"),
        "10_-7_5_div1024": ("no_grid", "no_grid", "no_grid", "no_grid", "no_grid"),
        "0_0_4096": ("no_grid", "no_grid", "no_grid", "no_grid", "no_grid"),
    },
    TIE_SCENE: {                                                    # B = 64, along_every_cap 262: every-ray rows per direction behind
        "unit": ("binned", "binned", "binned", "binned", "binned"),                     # 0 0 0 0 0
        "3_0_0": ("binned", "binned", "binned", "binned", "binned"),                    # 1 0 0 1 4
        "10_-7_5": ("binned", "binned", "binned", "binned", "binned"),                  # 4 6 0 3 5
        "300_200_-100": ("binned", "binned", "binned", "binned", "binned"),             # 58 154 144 78 96
        "1000_1000_1000": ("binned", "gave_up", "gave_up", "gave_up", "gave_up"),       # 198 483 519 291 301
        "origin_x1024": ("binned", "binned", "binned", "binned", "binned"),
        "origin_div1024": ("binned", "binned", "binned", "binned", "binned"),
        "40_-25_60_div1024": ("no_grid", "no_grid", "no_grid", "no_grid", "no_grid"),
        "10_-7_5_div1024": ("no_grid", "no_grid", "no_grid", "no_grid", "no_grid"),
        "0_0_4096": ("no_grid", "no_grid", "no_grid", "no_grid", "no_grid"),
    },
}
ALONG_BINS = {"soup33000": 256, TIE_SCENE: 64}                      # cells a side of the along grids; 32 for every other scene here

# The arbitrary-ray grid (grid/ray_grid.hpp) per scene and placement of GRID_PLACEMENTS: (class, plane-index pairs, every-ray rows), as
# tests/cpp/ray_grid_test.cpp's scene-file mode reports them from the header alone (test_ray_grid_host.py runs it again on every entry;
# never taken from a GPU).  `binned`: every-ray rows <= grid_every_cap(n) = max(n / 8, 64); `gave_up`: beyond it -- a plane bin's width
# no longer covers the rounding of the operands, so the triangle goes on the list of every ray; `no_grid`: no descriptor is made (none
# of these finite boxes is refused).  The counts of a structure that gave up are the program's, the library reports 0 for them.
RAY_GRID = {
    "soup2000": {                                                   # G = 16, cap 250
        "unit": ("binned", 4609, 1),
        "3_0_0": ("binned", 18923, 5),
        "10_-7_5": ("binned", 88414, 47),
        GRID_EDGE: ("binned", 251602, 213),
        "300_200_-100": ("gave_up", 0, 2000),
        "1000_1000_1000": ("gave_up", 0, 2000),
        "origin_x1024": ("binned", 4609, 1),
        "origin_div1024": ("binned", 4609, 1),
        "40_-25_60_div1024": ("gave_up", 0, 2000),
        "10_-7_5_div1024": ("gave_up", 0, 2000),
        "0_0_4096": ("gave_up", 0, 2000),
    },
    "cornell+soup2000": {                                           # G = 16, cap 253
        "unit": ("binned", 4739, 1),
        "3_0_0": ("binned", 19175, 5),
        "10_-7_5": ("binned", 90158, 47),
        GRID_EDGE: ("binned", 254912, 217),
        "300_200_-100": ("gave_up", 0, 2030),
        "1000_1000_1000": ("gave_up", 0, 2030),
        "origin_x1024": ("binned", 4739, 1),
        "origin_div1024": ("binned", 4739, 1),
        "40_-25_60_div1024": ("gave_up", 0, 2030),
        "10_-7_5_div1024": ("gave_up", 0, 2030),
        "0_0_4096": ("gave_up", 0, 2030),
    },
    TIE_SCENE: {                                                    # G = 32 (2100 triangles), cap 262: cells half as wide, given up sooner
        "unit": ("binned", 9874, 2),
        "3_0_0": ("binned", 59747, 32),
        "10_-7_5": ("gave_up", 298771, 279),
        GRID_EDGE: ("gave_up", 135527, 1725),
        "300_200_-100": ("gave_up", 0, 2100),
        "1000_1000_1000": ("gave_up", 0, 2100),
        "origin_x1024": ("binned", 9874, 2),
        "origin_div1024": ("binned", 9874, 2),
        "40_-25_60_div1024": ("gave_up", 0, 2100),
        "10_-7_5_div1024": ("gave_up", 0, 2100),
        "0_0_4096": ("gave_up", 0, 2100),
    },
}
RAY_GRID_CLASS = {scene: {p: row[0] for p, row in rows.items()} for scene, rows in RAY_GRID.items()}
RAY_GRID_CELLS = {"soup2000": 16, "cornell+soup2000": 16, TIE_SCENE: 32}
