"""The scope bank on the device: the cases the emulation runs (tests/scopebank_cases.py) against the reference's own ScopeVisualProcessor, one per
slot, and byte for byte against csdr_scope; and what only the device path has -- csdr_scopebank_process_bank behind a running pipeline against one
csdr_scope per slot fed csdr_bank_scope_frame, a slot's device spectrum points stepped into a waterfall where they lie, an execute issued straight
behind process_bank with no synchronise between, and one shape at size (256 slots, fftSize 1024)."""
import ctypes as C

import numpy as np
import pytest

import cubicsdr_amd.hip as H
from tests import scopebank_cases as K
from tests.test_gpu_io import TOL, _compare_scope_item, _need
from tests.util import demod_frequencies, synth_iq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from cubicsdr_amd.engine import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("L", K.SIZES)
def test_scopebank_against_the_reference(ctx, L):
    n, worst = K.check_against_reference(ctx, L)
    assert n == 2 * 7 * K.FRAMES and worst < K.TOL


@pytest.mark.parametrize("L", K.BYTE_SIZES + (4096,))
def test_scopebank_properties(ctx, L):
    K.check_properties(ctx, L)


@pytest.mark.parametrize("L", K.BYTE_SIZES)
def test_scopebank_refusals(ctx, L):
    from cubicsdr_amd.engine import DemodBank
    bank = DemodBank(ctx, 2, 1)
    try:
        K.check_refusals(ctx, L, bank)
    finally:
        bank.close()


# ----------------------------------------------------------------------------------------------- behind a pipeline
FS, M, BLOCK, CENTER, NB, NEXEC, L = 2400000, 4, 40000, 100000000, 2, 6, 1024
KINDS = [("NBFM", 12500), ("USB", 5400), ("AM", 100000), ("I/Q", 48000), ("FMS", 200000), ("QPSK", 200000), ("NBFM", 12500)]
N_SHOWN, AM_SLOT, QPSK_SLOT, OFF_SLOT = 5, 2, 5, 6


class _Pipeline:
    def __init__(self, ctx):
        from cubicsdr_amd.engine import DemodBank, ScopeBank, SDRPost
        freqs = demod_frequencies(CENTER, FS, len(KINDS))
        sig = ["NBFM", "USB", "AM", "NBFM", "FMS", "NBFM", "NBFM"]
        self.x = synth_iq(NEXEC * NB * BLOCK, FS, CENTER, list(zip(sig, freqs)), seed=77)
        self.post = SDRPost(ctx, FS, M, BLOCK, NB)
        self.bank = DemodBank(ctx, len(KINDS), NB)
        for i, ((k, bw), f) in enumerate(zip(KINDS, freqs)):
            if k == "QPSK":
                self.bank.configure_digital(i, self.post, k, bw, f)
            else:
                self.bank.configure(i, self.post, k, bw, f)
        self.bank.set_active(OFF_SLOT, False)
        self.sb = ScopeBank(ctx, L, 8, 1, 4096)          # (more slots than the bank has: the bank's count bounds the walk)

    def execute(self, e):
        self.post.execute(self.x[e * NB * BLOCK:(e + 1) * NB * BLOCK], NB, BLOCK, CENTER)
        self.bank.execute(self.post)

    def items(self):
        return K.items_of(self.sb)

    def close(self):
        for o in (self.sb, self.bank, self.post):
            o.close()


@pytest.fixture(scope="module")
def pipeline(ctx):
    """six executes, a process_bank and a full fetch behind each; per execute: the bank's items, one csdr_scope per shown slot fed
    csdr_bank_scope_frame, the AudioThreadInput the reference's statements would have assembled (tests/test_gpu_io.py), and the two waterfalls"""
    from cubicsdr_amd.engine import ScopeProcessor, Waterfall
    p = _Pipeline(ctx)
    scopes = [ScopeProcessor(ctx, L, max_frames=1, max_samples=4096) for _ in range(N_SHOWN)]
    wa, wb = Waterfall(ctx, L // 2, 8, 16), Waterfall(ctx, L // 2, 8, 16)
    lib = H.lib()
    rec = dict(bank=[], scope=[], inputs=[], rings=[])
    try:
        for e in range(NEXEC):
            p.execute(e)
            p.sb.process_bank(p.bank)
            rec["bank"].append(p.items())
            per_scope, per_input = [], []
            for i, (k, bw) in enumerate(KINDS[:N_SHOWN]):
                f = p.bank.scope_frame(i)
                assert f.n > 0, (e, k)
                scopes[i].process([f])
                per_scope.append((scopes[i].fetch(0, False), scopes[i].fetch(0, True)))
                r = p.bank.results(i)[-1]
                audio = p.bank.audio(i)[r.audio_offset:r.audio_offset + r.n_audio]
                if k == "I/Q":
                    n = min(audio.size, 4096)
                    per_input.append((np.concatenate([audio[1:n:2] * np.float32(0.75), audio[0:n:2] * np.float32(0.75)]), 2, 1, bw, bw))
                elif k == "FMS":
                    n = min(audio.size, 4096)
                    per_input.append((np.concatenate([audio[0:n:2], audio[1:n:2]]), 2, 1, 36000, 48000))
                elif r.n_audio > r.n_iq:
                    per_input.append((audio[:2048], 1, 0, bw, 48000))
                else:
                    per_input.append((p.bank.demod_output(i)[:2048], 1, 0, bw, bw))
            rec["scope"].append(per_scope)
            rec["inputs"].append(per_input)
            # the AM slot's spectrum (sample_rate == input_rate: L floats = L/2 pairs) into a waterfall of fft_size L/2: where it lies, and fetched
            ptr, n, stride = p.sb.device_points(AM_SLOT, True)
            assert n == 1 and stride == L
            taken = C.c_int()
            H.check(lib.csdr_waterfall_step(wa.h, C.c_void_p(ptr), 1, L, n, C.byref(taken)))
            wb.step(rec["bank"][-1][AM_SLOT][0][1]["points"].reshape(1, L))
            wa.update(); wb.update()
            rec["rings"].append([(wa.fetch_index(h), wb.fetch_index(h)) for h in range(2)])      # (the fetch also ends the waterfall's reads before the next process)
        yield rec
    finally:
        for o in scopes + [wa, wb]:
            o.close()
        p.close()


def test_process_bank_is_a_scope_per_slot(pipeline):
    """NBFM, USB (audio taps), AM at 100 kHz (the n_dev tap), I/Q, FM stereo (both stereo layouts read in place): byte for byte one csdr_scope per
    slot fed bank.scope_frame(i); the QPSK and the inactive slot get no frames; the AM slot's device points give the ring the fetched points give"""
    for e in range(NEXEC):
        got = pipeline["bank"][e]
        for i in range(N_SHOWN):
            assert K.same_bytes(got[i], [pipeline["scope"][e][i]]), (e, KINDS[i])
        assert not got[QPSK_SLOT] and not got[OFF_SLOT] and not got[7], e
        assert got[AM_SLOT][0][1]["points"].size == L and got[AM_SLOT][0][0]["points"].size == 2 * 1024
        for h, (a, b) in enumerate(pipeline["rings"][e]):
            assert np.array_equal(a, b), (e, h)
    assert pipeline["rings"][-1][0][0].any()
    assert pipeline["bank"][0][3][0][0]["mode"] == 1 and pipeline["bank"][0][4][0][1]["points"].size == 2 * 384      # stereo: 2Y; FMS labelled 36000 / 48000


def test_process_bank_against_the_reference(pipeline):
    import oracle.ref_modems as RM
    _need(RM.scope_available(), "libref_scope.so")
    refs = [RM.RefScopeCpp(L) for _ in range(N_SHOWN)]
    worst = 0.0
    try:
        for e in range(NEXEC):
            for i, (k, _) in enumerate(KINDS[:N_SHOWN]):
                data, ch, typ, sr, ir = pipeline["inputs"][e][i]
                want = refs[i].push(data, ch, ir, sr, typ)
                wave, spec = pipeline["bank"][e][i][0]
                _compare_scope_item(wave, want[0], (e, k, "wave"))
                err = _compare_scope_item(spec, want[1], (e, k, "spectrum"))
                print("scope bank behind the pipeline, execute %d %s: spectrum rel_err %.3g" % (e, k, err))
                assert err < TOL, (e, k, err)
                worst = max(worst, err)
    finally:
        for r in refs:
            r.close()
    print("scope bank behind the pipeline: worst spectrum error %.3g" % worst)


def test_the_next_execute_waits_for_the_reader(ctx, pipeline):
    """the same pipeline again, with execute e + 1 issued straight behind process_bank of execute e -- no synchronise between -- and the items of
    batch e fetched only then: the single-buffered taps were not rewritten under the reader, the items are the synchronised run's byte for byte"""
    p = _Pipeline(ctx)
    try:
        p.execute(0)
        for e in range(NEXEC):
            p.sb.process_bank(p.bank)
            if e + 1 < NEXEC:
                p.execute(e + 1)
            got = p.items()
            for i in range(8):
                assert K.same_bytes(got[i], pipeline["bank"][e][i]), (e, i)
    finally:
        p.close()


# ----------------------------------------------------------------------------------------------- at size
def test_256_slots_at_size(ctx):
    """256 slots, fftSize 1024, one frame of 800 +- 1 samples per slot and call, three calls: eight sampled slots byte for byte against a csdr_scope
    each and against a second bank fed only them"""
    from cubicsdr_amd.engine import ScopeBank, ScopeProcessor
    S, NC = 256, 3
    rng = np.random.default_rng(11)
    t = np.arange(801)
    calls = []
    for c in range(NC):
        call = []
        for s in range(S):
            n = 800 + int(rng.integers(-1, 2))
            data = ((0.2 + 0.003 * s) * np.sin(2 * np.pi * (300 + 11 * s + 50 * c) * t[:n] / 48000.0) + 0.01 * rng.standard_normal(n)).astype(np.float32)
            call.append((s, dict(data=data, channels=1, type=0, sample_rate=12500, input_rate=48000)))
        calls.append(call)
    sampled = (0, 1, 63, 64, 127, 128, 200, 255)
    full, few = ScopeBank(ctx, L, S, 1, 1024), ScopeBank(ctx, L, S, 1, 1024)
    scopes = {s: ScopeProcessor(ctx, L, max_frames=1, max_samples=1024) for s in sampled}
    try:
        for c, call in enumerate(calls):
            full.process(call)
            few.process([it for it in call if it[0] in sampled])
            assert [full.frames(s) for s in range(S)] == [1] * S
            assert [few.frames(s) for s in range(S)] == [1 if s in sampled else 0 for s in range(S)]
            for s in sampled:
                scopes[s].process([call[s][1]])
                want = [(scopes[s].fetch(0, False), scopes[s].fetch(0, True))]
                a = [(full.fetch(s, 0, False), full.fetch(s, 0, True))]
                b = [(few.fetch(s, 0, False), few.fetch(s, 0, True))]
                assert K.same_bytes(a, want) and K.same_bytes(b, want), (c, s)
                assert a[0][1]["points"].size == 2 * 133
    finally:
        for o in [full, few] + list(scopes.values()):
            o.close()
