"""The waterfall raster on the device, bit for bit against the numpy model of tests/waterfall_cases.py: the cases the emulation runs, the quantiser
over EVERY float32 bit pattern in [0, 1] plus the specials (the expected bytes computed by torch in float64 on the device, independent of the
kernel), and a 512-line ring at fftSize 65536 fed from a spectrum's contiguous frames in HBM over three calls, with updates that cross the wrap."""
import numpy as np
import pytest

from tests import waterfall_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from cubicsdr_amd.engine import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("pair", [False, True], ids=["plain", "pairs"])
@pytest.mark.parametrize("fft_size", K.FFT_SIZES)
def test_quantiser_specials(ctx, fft_size, pair):
    assert K.check_quantiser_specials(ctx, fft_size, pair) > 3000


@pytest.mark.parametrize("exponent", [-1, -8])
def test_quantiser_whole_binade(ctx, exponent):
    assert K.check_quantiser_binade(ctx, exponent) == 1 << 23


def torch_quantise(v):
    """the header's rule in float64 on the device"""
    import torch
    v64 = v.double()
    c = torch.tensor(0.99, dtype=torch.float32, device=v.device)
    wv = torch.where(v < 0, torch.zeros_like(v), torch.where(v64 > 0.99, c, v))
    wv = torch.where(torch.isnan(v), torch.zeros_like(v), wv)
    return torch.floor(wv.double() * 255.0).to(torch.uint8)


@pytest.mark.parametrize("pair", [False, True], ids=["plain", "pairs"])
def test_quantiser_every_float_in_0_1(ctx, pair):
    import torch
    dev = torch.device("cuda:0")
    fft_size, chunk = 65536, 1 << 24
    last = 0x3F800000                                         # 1.0f
    seen = np.zeros(256, np.int64)
    total = 0
    starts = list(range(0, last + 1, chunk))
    if pair:
        starts = starts[::8] + starts[-2:]                   # the pair layout shares the arithmetic: every eighth chunk and the end of the range
    for start in starts:
        end = min(start + chunk, last + 1)
        bits = torch.arange(start, end, dtype=torch.int64, device=dev).to(torch.int32)
        if end == last + 1:                                   # the specials ride along with the last chunk
            sp = torch.from_numpy(K.special_values().view(np.int32)).to(dev)
            bits = torch.cat([bits, sp])
        v = bits.view(torch.float32)
        got, n_lines, half = K.quantise_through_panel(ctx, v, fft_size, pair, device=True)
        want = torch_quantise(v).cpu().numpy()
        got = got.reshape(-1)[:want.size]
        assert np.array_equal(got, want), (hex(start), np.argwhere(got != want)[:8])
        seen += np.bincount(want, minlength=256)
        total += want.size
    assert total >= (last + 1 if not pair else 9 * chunk)
    assert seen[:253].all() and not seen[253:].any()          # every index up to 252 occurs, none above


def test_worked_example(ctx):
    K.check_worked_example(ctx)
    K.check_worked_example(ctx, 65536)


@pytest.mark.parametrize("pair", [False, True], ids=["plain", "pairs"])
@pytest.mark.parametrize("fft_size", K.FFT_SIZES + (65536,))
def test_life_cycle_and_ring(ctx, fft_size, pair):
    K.check_life_cycle(ctx, fft_size, pair)


@pytest.mark.parametrize("fft_size", K.FFT_SIZES + (4096,))
def test_rgba(ctx, fft_size):
    K.check_rgba(ctx, fft_size)


@pytest.mark.parametrize("hide_dc", [False, True], ids=["plain", "hide_dc"])
@pytest.mark.parametrize("fft_size,bandwidth", [(1024, 240000), (600, None)])
def test_step_spec(ctx, fft_size, bandwidth, hide_dc):
    K.check_step_spec(ctx, fft_size, hide_dc, bandwidth)


def test_device_points_and_device_picture(ctx):
    """lines that lie in HBM (a torch tensor) and a picture that stays there: read back with torch, equal to the fetched one"""
    import torch
    from cubicsdr_amd.engine import Waterfall
    fft_size, lines = 4096, 9
    rng = np.random.default_rng(5)
    a = rng.uniform(-0.2, 1.2, (6, fft_size)).astype(np.float32)
    wf = Waterfall(ctx, fft_size, lines, max_pending=8)
    m = K.PanelModel(fft_size, lines)
    try:
        wf.step(None); wf.update(); m.step(); m.update()
        t = torch.from_numpy(a).to("cuda:0")
        torch.cuda.synchronize()
        assert wf.step(t) == 6
        for row in a:
            m.set_points(row)
            m.step()
        wf.update(); m.update()
        wf.set_gradient(K.STOPS5)
        want = m.rgba(K.np_table(K.STOPS5), 0, lines)
        assert np.array_equal(wf.fetch_rgba(0, lines), want)
        wf.fetch_rgba(0, lines, fetch=False)
        ptr = wf.device_rgba()
        ctx.synchronize()
        from cubicsdr_amd import hip as H
        import ctypes as C
        back = np.empty(want.shape, np.uint8)
        H.check(H.lib().csdr_dev_download(ctx.h, back.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), back.size))
        assert np.array_equal(back, want)
    finally:
        wf.close()


def test_ring_512_lines_from_a_spectrum_of_65536(ctx):
    """the benchmark's spectrum shape: contiguous frames of fftSize 65536 at 61.44 MS/s, hideDC on, 3 x 200 frames stepped HBM to HBM into a 512-line ring;
    the third update crosses the wrap.  Textures and offsets against the model fed with what csdr_spec_fetch returns."""
    import torch
    from cubicsdr_amd.engine import SpectrumProcessor, Waterfall
    F, lines, nf, fs, center = 65536, 512, 200, 61440000, 100000000
    sp = SpectrumProcessor(ctx, F, max_frames=nf)
    wf = Waterfall(ctx, F, lines, max_pending=256)
    m = K.PanelModel(F, lines)
    try:
        sp.set_hide_dc(True, center_freq=center, bandwidth=fs, input_freq=center)
        wf.set_gradient(K.STOPS5)
        wf.step(None); wf.update(); m.step(); m.update()
        g = torch.Generator(device="cuda:0").manual_seed(65536)
        tone = torch.exp(2j * np.pi * 0.0371 * torch.arange(nf * 2 * F, device="cuda:0", dtype=torch.float64)).to(torch.complex64)
        for call in range(3):
            x = (torch.randn(nf * 2 * F, 2, device="cuda:0", generator=g) * 0.05).contiguous()
            x = (torch.view_as_complex(x) + (0.2 + 0.1 * call) * tone + 0.3).contiguous()
            torch.cuda.synchronize()
            assert sp.process(x, 1, nf * 2 * F, contiguous=True) == nf
            assert wf.step_spec(sp, 0, nf) == nf
            wf.update()
            for f in range(nf):
                m.set_points(sp.fetch(f)[0])
                assert m.step() == 1
            m.update()
            assert wf.offset(0) == m.ofs[0] and wf.offset(1) == m.ofs[1]
        assert m.ofs[0] == 511 - 600 + 512
        for j in range(2):
            got = wf.fetch_index(j)
            assert np.array_equal(got, m.tex[j]), np.argwhere(got != m.tex[j])[:8]
            assert len(np.unique(got)) > 20
        want = m.rgba(K.np_table(K.STOPS5), 500, 12)
        assert np.array_equal(wf.fetch_rgba(500, 12), want)
    finally:
        wf.close()
        sp.close()
