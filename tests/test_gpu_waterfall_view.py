"""The waterfall's viewport on the device, bit for bit: the cases the emulation runs (tests/waterfall_view_cases.py), and one view at workload scale --
fftSize 65536, a 512-line ring of random index lines stepped from a torch tensor, viewed at 1920 x 400 in both modes, the expected picture computed
with torch on the device and the picture read back through torch from the pointer csdr_waterfall_device_view hands out."""
import numpy as np
import pytest

from tests import waterfall_view_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from cubicsdr_amd.engine import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("lines", K.LINES)
@pytest.mark.parametrize("fft_size", K.FFT_SIZES)
def test_views(ctx, fft_size, lines):
    assert K.check_views(ctx, fft_size, lines) == (7 + 2 + 2) * 5 * 2


@pytest.mark.parametrize("fft_size,lines", [(16, 7), (30, 12), (601, 7), (2048, 12)])
def test_view_properties(ctx, fft_size, lines):
    K.check_view_properties(ctx, fft_size, lines)


def test_wide_footprints(ctx):
    K.check_wide_footprints(ctx)


def torch_view(tex, ofs, table, fft_size, W, Hh, mode):
    """the header's items 3 and 4 with torch on the device; tex: [2, L, half] uint8, table: [256, 4] uint8 -> [Hh, W, 4] uint8"""
    import torch
    dev = tex.device
    L, half = int(tex.shape[1]), int(tex.shape[2])
    ct, rt = K.np_columns(fft_size, W, mode), K.np_rows(L, Hh, mode)
    t = lambda a, dt=torch.int64: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt)
    hh, cf, cc = t(ct["half"]), t(ct["first"]), t(ct["count"])
    rf, rc = t(rt["first"]), t(rt["count"])
    if mode == K.PEAK:
        best = torch.zeros((Hh, W), dtype=torch.uint8, device=dev)
        for dr in range(int(rc.max())):
            rows = (ofs + rf + torch.minimum(torch.full_like(rc, dr), rc - 1)) % L
            for dc in range(int(cc.max())):
                cols = cf + torch.minimum(torch.full_like(cc, dc), cc - 1)
                best = torch.maximum(best, tex[hh[None, :], rows[:, None], cols[None, :]])
        return table[best.long()]
    j0 = (ofs + rf + L) % L
    j1 = (j0 + 1) % L
    colour = lambda j, i: table[tex[hh[None, :], j[:, None], i[None, :]].long()][..., :3].float()
    c00, c10, c01, c11 = colour(j0, cf), colour(j0, cf + 1), colour(j1, cf), colour(j1, cf + 1)
    al, be = t(ct["frac"], torch.float32)[None, :, None], t(rt["frac"], torch.float32)[:, None, None]
    top = c00 + al * (c10 - c00)                            # eager float32 tensors: every operation is rounded on its own
    bot = c01 + al * (c11 - c01)
    m = top + be * (bot - top)
    out = torch.full((Hh, W, 4), 255, dtype=torch.uint8, device=dev)
    out[..., :3] = (m + 0.5).to(torch.uint8)
    return out


class DevicePicture:
    """a picture in HBM as torch takes it in (torch.as_tensor, no copy)"""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "|u1", "data": (int(ptr), False), "version": 2, "strides": None}


def test_ring_of_65536_by_512_viewed_at_1920_by_400():
    import torch
    from cubicsdr_amd.engine import Context, Waterfall
    from tests.waterfall_cases import STOPS5, np_table
    F, lines, W, Hh = 65536, 512, 1920, 400
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1920)
    ctx = Context(0, torch.cuda.current_stream().cuda_stream)      # torch reads the picture in HBM: its stream is the boundary stream
    wf = Waterfall(ctx, F, lines, max_pending=256)
    try:
        wf.set_gradient(STOPS5)
        wf.step(None); wf.update()
        for n in (256, 256, 88):                            # 600 lines: the ring goes round and the last update crosses the wrap
            idx = torch.randint(0, 253, (n, F), device=dev, generator=g)
            idx[:, 4099] = 252                              # a carrier one bin wide
            v = ((idx.float() + 0.5) / 255.0).contiguous()   # the middle of index idx's interval
            assert wf.step(v) == n                           # (made on the boundary stream: the step is ordered behind it)
            wf.update()
        ofs = wf.offset(0)
        assert ofs == 511 - 600 + 512
        tex = torch.from_numpy(np.stack([wf.fetch_index(0), wf.fetch_index(1)])).to(dev)
        assert int(tex.max()) == 252 and len(torch.unique(tex)) == 253
        table = torch.from_numpy(np_table(STOPS5)).to(dev)
        for name, mode in K.MODES:
            want = torch_view(tex, ofs, table, F, W, Hh, mode)
            got = wf.view(W, Hh, name)
            assert np.array_equal(got, want.cpu().numpy()), (name, np.argwhere(got != want.cpu().numpy())[:8])
            # the picture that stays on the device, read through torch on the boundary stream: no host synchronisation in between
            wf.view(W, Hh, name, fetch=False)
            ptr, w, h = wf.device_view()
            assert (w, h) == (W, Hh)
            there = torch.as_tensor(DevicePicture(ptr, (Hh, W, 4)), device=dev)
            assert torch.equal(there, want), name
        # the carrier: PEAK keeps it in every row, LINEAR (2 x 2 texels out of 34 x 1.28) does not
        px = 4099 * (W // 2) // (F // 2)
        carrier = np_table(STOPS5)[252, :3]
        assert (wf.view(W, Hh, "peak")[:, px, :3] == carrier).all()
        assert not (wf.view(W, Hh, "linear")[:, px, :3] == carrier).all()
    finally:
        wf.close()
        ctx.close()
