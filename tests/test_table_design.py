"""csdr_design_rings (host only) against the reference binary's own APSK descriptions, which it exports as data: from the points of the binary's
modulator alone the design gives the binary's rings, ring sizes and symbol map exactly, phases of 0, and radii and slicers within 1e-6 (the
digital lab's EVM floor).  And the refusals.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import cubicsdr_amd.hip as H
from tests import table_oracle as T

pytestmark = pytest.mark.skipif(not T.available(), reason="the oracle (oracle/_ref) is not built: run __graft_entry__.build()")


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    from cubicsdr_amd import build
    build.build(verbose=False)
    return T.Libs(tmp_path_factory.mktemp("table_shim"))


@pytest.mark.parametrize("name", T.APSK)
def test_design_rings_reproduces_the_binary(libs, name):
    from cubicsdr_amd.engine import design_rings
    pts = T.constellation(libs, name)
    want = T.apsk_description(libs, name)
    c = design_rings(pts)
    L = c.n_rings
    assert c.rule == H.CSDR_TABLE_RINGS and c.n_points == pts.size
    assert L == want["p"].size
    assert list(c.ring_size[:L]) == list(want["p"])
    assert list(c.ring_map[:pts.size]) == list(want["map"])
    assert all(v == 0.0 for v in c.ring_phase[:L]) and not want["phi"].any()
    dr = np.abs(np.array(c.ring_radius[:L], np.float64) - want["r"])
    ds = np.abs(np.array(c.ring_slicer[:L - 1], np.float64) - want["slicer"]) if L > 1 else np.zeros(1)
    print("design_rings %-8s rings %s: max |radius - r| %.3g, max |slicer - r_slicer| %.3g" % (name, list(want["p"]), dr.max(), ds.max()))
    assert dr.max() <= 1e-6 and ds.max() <= 1e-6, (name, dr, ds)
    assert np.array_equal(np.array(c.points[:2 * pts.size], np.float32), pts.view(np.float32))


def _rc(points):
    x = np.ascontiguousarray(points, dtype=np.complex64)
    return H.lib().csdr_design_rings(x.ctypes.data_as(C.c_void_p), int(x.size), C.byref(H.Constellation()))


def test_design_rings_refusals(libs):
    pts = T.constellation(libs, "APSK16")
    assert _rc(pts) == 0
    ring12 = np.exp(2j * np.pi * np.arange(12) / 12).astype(np.complex64)
    assert _rc(ring12) == -1                                                    # 12 points
    assert _rc(np.exp(2j * np.pi * np.arange(512) / 512)) == -1                 # 512 points
    dup = pts.copy()
    dup[5] = dup[9]
    assert _rc(dup) == -1                                                       # two equal points
    for k in (0, 7, 15):                                                        # a ring with one point moved by 1e-2: along the ring, then outwards
        for delta in (np.exp(1j * 1e-2), 1 + 1e-2 / abs(pts[k])):
            moved = pts.copy()
            moved[k] = moved[k] * delta
            assert _rc(moved) == -1, (k, delta)
    assert _rc(np.zeros(16, np.complex64)) == -1
