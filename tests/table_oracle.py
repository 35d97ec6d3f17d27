"""TEST INFRASTRUCTURE ONLY: the reference binary's APSK / SQAM / V.29 / arb modem objects as the parity oracle of the table-driven slots.

tests/digital/liquid_table_shim.c is compiled at test time like liquid_digital_shim.c (whose modemcf wrappers drive every object here); it adds
modemcf_create_arbitrary and a reader of the binary's exported APSK descriptions.  The constellation handed to the product is always what the
binary's own modemcf_modulate returns, symbol by symbol: no point, ring constant or map of liquid is stored in the repository.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import digital_oracle as O

SHIM_SRC = os.path.join(O.HERE, "digital", "liquid_table_shim.c")

# liquid's modulation_scheme values (name -> (scheme, points))
SCHEMES = {"APSK4": (32, 4), "APSK8": (33, 8), "APSK16": (34, 16), "APSK32": (35, 32), "APSK64": (36, 64), "APSK128": (37, 128), "APSK256": (38, 256),
           "SQAM32": (42, 32), "SQAM128": (43, 128), "V29": (44, 16),
           "ARB16OPT": (45, 16), "ARB32OPT": (46, 32), "ARB64OPT": (47, 64), "ARB128OPT": (48, 128), "ARB256OPT": (49, 256), "ARB64VT": (50, 64)}
APSK = [n for n in SCHEMES if n.startswith("APSK")]
USER = "USER64"                       # a seeded 64-point table of the caller's through modemcf_create_arbitrary
NAMES = list(SCHEMES) + [USER]
SENSITIVITY = 0.005                   # ModemAPSK / ModemSQAM / ModemST: updateDemodulatorLock(mod, 0.005f)

available = O.available
_shim = None


def shim(build_dir):
    """compile (once per process) and load the table shim; build_dir: a writable scratch directory"""
    global _shim
    if _shim is None:
        out = os.path.join(str(build_dir), "libliquid_table_shim.so")
        subprocess.run([os.environ.get("CC", "gcc"), "-O2", "-fPIC", "-shared", SHIM_SRC, "-o", out, "-L" + O.REF_DIR, "-lliquid_ref",
                        "-Wl,-rpath," + O.REF_DIR], check=True)
        lib = C.CDLL(out)
        p, i = C.c_void_p, C.c_int
        for name, (res, args) in {"shim_table_ready": (i, []), "shim_modem_create_arbitrary": (p, [p, i]),
                                  "shim_apsk_read": (i, [i, p, p, p, p, p])}.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        assert lib.shim_table_ready(), "the reference binary lacks modemcf_create_arbitrary or a liquid_apsk export"
        _shim = lib
    return _shim


class Libs:
    """the two shims: d = liquid_digital_shim (modemcf objects), t = liquid_table_shim"""

    def __init__(self, build_dir):
        self.d, self.t = O.shim(build_dir), shim(build_dir)


def user_points(seed=20):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, 64) + 1j * rng.uniform(-1, 1, 64)).astype(np.complex64)


def n_points(name):
    return 64 if name == USER else SCHEMES[name][1]


class Modem(O.Modem):
    """one modemcf object of the reference binary, by scheme name (USER64: modemcf_create_arbitrary on the seeded table)"""

    def __init__(self, libs, name):
        self.lib = libs.d
        if name == USER:
            pts = user_points()
            self.q = libs.t.shim_modem_create_arbitrary(pts.ctypes.data_as(C.c_void_p), pts.size)
        else:
            self.q = libs.d.shim_modem_create(SCHEMES[name][0])
        assert self.q, name


def constellation(libs, name):
    """every point of the object's constellation, by symbol, from its own modulator (arb_init rescales a caller's table)"""
    m = Modem(libs, name)
    pts = m.modulate(np.arange(n_points(name), dtype=np.uint32))
    m.close()
    return pts


def apsk_description(libs, name):
    """the binary's exported description of an APSK scheme: dict of p, r, phi, slicer, map"""
    M = SCHEMES[name][1]
    p, r, phi, sl = np.zeros(8, np.uint32), np.zeros(8, np.float32), np.zeros(8, np.float32), np.zeros(8, np.float32)
    mp = np.zeros(256, np.uint8)
    L = libs.t.shim_apsk_read(M, *(a.ctypes.data_as(C.c_void_p) for a in (p, r, phi, sl, mp)))
    assert L, name
    return {"p": p[:L].astype(int), "r": r[:L], "phi": phi[:L], "slicer": sl[:L - 1], "map": mp[:M].astype(int)}


def product_table(name, pts):
    """the H.Constellation a binding would hand over: APSK through csdr_design_rings, SQAM nearest-point behind the quadrant fold, everything
    else nearest-point"""
    from cubicsdr_amd.engine import design_rings, nearest_table
    return design_rings(pts) if name.startswith("APSK") else nearest_table(pts, quadrant=name.startswith("SQAM"))


def boundary_mask(libs, name, x, ref_syms, rel=1e-6):
    """samples whose reference decision moves under digital_oracle.perturbed_runs' eight perturbations of `rel` relative"""
    x = np.asarray(x, dtype=np.complex64)
    a = np.abs(x).astype(np.float32)
    mask = np.zeros(ref_syms.size, bool)
    for d in (x * (1 + rel), x * (1 - rel), x * (1 + 1j * rel), x * (1 - 1j * rel), x + rel * a, x - rel * a, x + 1j * rel * a, x - 1j * rel * a):
        m = Modem(libs, name)
        mask |= m.demodulate(d.astype(np.complex64)) != ref_syms
        m.close()
    return mask


def nearest_restated(pts, x):
    """the first nearest point in float32 -- the rule that is NOT modemcf_demodulate_apsk's"""
    x = np.asarray(x, np.complex64)
    dx = (x.real[:, None] - pts.real[None, :]).astype(np.float32)
    dy = (x.imag[:, None] - pts.imag[None, :]).astype(np.float32)
    return np.argmin((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32), axis=1).astype(np.uint32)


class RefTable:
    """ModemAPSK / ModemSQAM / ModemST around the binary's objects, block by block: one object per "cons", all created up front, switched by
    writeSetting("cons"), updateDemodulatorLock(mod, 0.005) after each block"""

    def __init__(self, libs, names):
        self.objs = {n_points(n): Modem(libs, n) for n in names}
        self.cons = n_points(names[0])
        self.lock = False

    def set_cons(self, cons):
        assert cons in self.objs
        self.cons = cons

    def demodulate(self, x):
        m = self.objs[self.cons]
        syms = m.demodulate(np.asarray(x, dtype=np.complex64))
        evm = m.evm()
        self.lock = evm <= np.float32(SENSITIVITY)
        return syms, evm

    def close(self):
        for m in self.objs.values():
            m.close()
        self.objs = {}
