"""GPU: the sample kernel (emu_amd/csrc/sample.hip) through ``emu_sample_bf16`` against its specification emu_amd/sampling.py.

Shapes: V = 97 (less than one wave's stride), 1000 (no multiple of 8 or 64), 4099 (prime, more than 1024 threads x 4), 32 274 (the
model's own); 1, 5 and 64 rows; rows ``V`` and ``V + 3`` elements apart with the base pointer one element (2 bytes) off any wider
alignment.  The inputs and their screened seeds are tests/sampler_cases.py's; 64 rows are the 5 screened rows repeated.
"""
import functools

import pytest
import torch

from emu_amd import sampling
from tests import sampler_cases as sc

pytestmark = pytest.mark.gpu

ROWS = (1, 5, 64)
GRID = [(V, R, pad) for V in sc.VOCABS for R in ROWS for pad in (0, 3)]
PAD_ID, NO_EOS = 1, -1


def _params(o, do_sample=True, eos_id=NO_EOS, pad_id=PAD_ID, min_len=1 << 30):
    from emu_amd.llama import sample_params
    return sample_params(do_sample, o.get("temperature"), o.get("top_k"), o.get("top_p"), o.get("repetition_penalty", 1.0),
                         o.get("suppress_id"), min_len, eos_id, pad_id, o.get("min_keep", 1))


def _strided(x, pad):
    """x [R, V] on the device in rows V + pad apart, the base one element past an aligned address."""
    R, V = x.shape
    buf = torch.zeros(R * (V + pad) + 1, dtype=torch.bfloat16, device="cuda")
    view = torch.as_strided(buf, (R, V), (V + pad, 1), storage_offset=1)
    view.copy_(x)
    assert view.data_ptr() % 4 == 2 and view.stride(0) == V + pad
    return view


def _hist(o, R):
    """(hist int32 [steps, R] on the device, step count) of a case's history, rows repeated to R."""
    h = o.get("history")
    if h is None:
        return None, 0
    h = h[torch.arange(R) % h.shape[0]]
    hist = torch.empty(h.shape[1], R, dtype=torch.int32, device="cuda")
    hist.copy_(h.t())
    return hist, h.shape[1]


def _run(view, o, step, do_sample=True, uniforms=None, unfinished=None, probs=False, hist=None, eos_id=NO_EOS, min_len=1 << 30):
    from emu_amd import ops
    R, V = view.shape
    step_dev = torch.tensor([step], dtype=torch.int32, device="cuda")
    if do_sample and uniforms is None:
        uniforms = torch.full((max(step, 0) + 1, R), 0.5, dtype=torch.float32, device="cuda")
    pr = torch.full((R, V), -1.0, dtype=torch.float32, device="cuda") if probs else None
    out = ops.sample(view, step_dev, _params(o, do_sample, eos_id, min_len=min_len), hist=hist, uniforms=uniforms,
                     unfinished=unfinished, probs_out=pr)
    torch.cuda.synchronize()
    return out.cpu().long(), (pr.cpu() if probs else None)


@functools.lru_cache(maxsize=None)
def _spec(V, name):
    """Computed once per case: (logits [5, V] bf16, options, probabilities fp32, probabilities fp64), never modified."""
    x, o = sc.case(V, name)
    return x, o, sampling.reference_probs(x, **o), sampling.reference_probs(x, dtype=torch.float64, **o)


@pytest.mark.parametrize("V,R,pad", GRID)
def test_greedy_mode(V, R, pad):
    """No penalty: the ids of ``emu_argmax_bf16`` bit for bit (first index of a tied maximum included).  With a penalty over a
    history with duplicates, an id >= V and a row without usable ids, and with a suppressed id: the spec's first-index arg-max.  The
    empty history (step 0) changes nothing."""
    from emu_amd import ops
    x = sc.rows(V, 5)[torch.arange(R) % sc.ROWS].clone()
    x[:, 40] = x[:, 3] = x.float().max() + 1                # a tied maximum: index 3 wins
    view = _strided(x, pad)
    got, _ = _run(view, {}, 0, do_sample=False)
    assert got.tolist() == ops.argmax(view).cpu().tolist() == [3] * R
    o = dict(repetition_penalty=1.3, history=sc.history(V), suppress_id=3)
    x[:, 5] = x[:, 3]                                       # penalised in row 0 (id 5 is in its history), first index among equals elsewhere
    view = _strided(x, pad)
    hist, n = _hist(o, R)
    want = sampling.reference_greedy(x, o["history"][torch.arange(R) % sc.ROWS], 1.3, suppress_id=3)
    got, _ = _run(view, o, n, do_sample=False, hist=hist, min_len=n + 1)
    assert got.tolist() == want.tolist()
    assert len(set(want.tolist())) > 1 or R == 1            # the penalty moved some row's choice
    got0, _ = _run(view, o, 0, do_sample=False, hist=hist, min_len=0)       # step 0: no history in use, suppress expired
    assert got0.tolist() == ops.argmax(view).cpu().tolist()


@pytest.mark.parametrize("V,R,pad", GRID)
def test_kept_set_and_probabilities(V, R, pad):
    """``probs_out > 0`` is exactly the spec's kept set and the values agree within 1e-5, for every option set of
    tests/sampler_cases.py: top_k in {1, 50, V + 10}, top_p in {0.05, 0.9, 1.0}, both, min_keep = 2 under a top_p that keeps
    nothing else, temperature in {0.7, 1.0, 2.0}, a repetition penalty, a suppressed id."""
    idx = torch.arange(R) % sc.ROWS
    for name in sc.CASES:
        x, o, q32, q64 = _spec(V, name)
        hist, n = _hist(o, R)
        tok, pr = _run(_strided(x[idx], pad), o, n, probs=True, hist=hist)
        assert torch.equal(pr > 0, q32[idx] > 0), name
        err = float((pr.double() - q64[idx]).abs().max())
        print(f"V={V} rows={R} ld=V+{pad} {name}: kept {int((pr[0] > 0).sum())}, max |q - spec| {err:.2e}")
        assert err <= 1e-5, (name, err)
        assert bool((q32[idx].gather(1, tok[:, None]) > 0).all()), name        # the token drawn at u = 0.5 is a kept one
        if name == "mk2":
            assert (pr > 0).sum(dim=1).tolist() == [2] * R


# the draw's tolerance: derived in test_draw_lies_in_the_reference_interval's docstring
DRAW_TOL = (52 + 50 + 1) * 2.0 ** -24 + 2 * (2.0 ** -22 + 2.0 ** -24 * 10.6)


@pytest.mark.parametrize("V,name", [(1000, "p1"), (1000, "t07"), (32274, "p1"), (32274, "both"), (32274, "t20"), (4099, "pen")])
def test_draw_lies_in_the_reference_interval(V, name):
    """64 rows of ONE logit row under 64 different uniforms, u = 0 and u = 1 - 2^-24 among them: the kernel's token t passes iff u
    lies in [lo_t - tol, hi_t + tol] of the fp64 intervals.  Every draw is judged, none is left out.

    tol = DRAW_TOL, from the kernel's summation shape (sample.hip).  A term of a cumulative value passes at most 40 sequential
    adds inside its thread's chunk (chunks hold at most 41 ids), 6 levels of the scan inside the wave, 4 levels of the scan over the 16
    wave totals and 2 more adds (wave prefix + lane prefix, + the chunk's own prefix): 52 roundings of at most 2^-24 relative each; a
    term of the normaliser at most 40 + 6 + 4 = 50; u * total rounds once more.  The terms themselves are exp(s - max) in fp32: the
    subtraction is off by at most 2^-24 |d| absolutely, which is that much relatively in exp, and expf by at most 2 ulp = 2^-22; summed
    with the weights q_i that is at most 2^-22 + 2^-24 * sum q_i |d_i| <= 2^-22 + 2^-24 ln V in the numerator and again in the
    normaliser.  With V <= 40 000: (52 + 50 + 1) * 2^-24 + 2 * (2^-22 + 2^-24 * 10.6) = 6.14e-6 + 1.74e-6 = 7.9e-6 < 1e-5.
    """
    assert DRAW_TOL < 1e-5
    x, o, q32, q64 = _spec(V, name)
    R = 64
    g = torch.Generator().manual_seed(V)
    u = torch.rand(R, generator=g, dtype=torch.float32)
    u[0], u[1] = 0.0, 1 - 2.0 ** -24
    hist, n = _hist(o, sc.ROWS)
    if hist is not None:
        hist = hist[:, :1].expand(-1, R).contiguous()
    uni = torch.zeros(n + 1, R)
    uni[n] = u
    tok, _ = _run(_strided(x[:1].expand(R, V), 3), o, n, uniforms=uni.cuda(), hist=hist)
    lo, hi = sampling.reference_intervals(q64[:1])
    lo_t, hi_t = lo[0, tok], hi[0, tok]
    ud = u.double()
    worst = float(torch.maximum(lo_t - ud, ud - hi_t).max())
    print(f"V={V} {name}: distinct tokens {tok.unique().numel()}, worst distance outside the interval {worst:.2e} (tol {DRAW_TOL:.2e})")
    assert bool((q64[0, tok] > 0).all())
    assert bool(((ud >= lo_t - DRAW_TOL) & (ud <= hi_t + DRAW_TOL)).all()), worst
    assert int(tok[0]) == int((q64[0] > 0).nonzero()[0])    # u = 0: the lowest kept id


def test_bookkeeping_flags_and_pad():
    """A row whose flag is 0 emits pad_id whatever its logits and stays 0; a row that draws eos_id has its flag cleared; the other
    rows' flags are untouched.  Greedy mode keeps the same books."""
    V = 1000
    x, o, q32, _ = _spec(V, "both")
    view = _strided(x, 0)
    free, _ = _run(view, o, 0)
    eos = int(free[2])
    for do_sample in (True, False):
        flags = torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32, device="cuda")
        base, _ = _run(view, o, 0, do_sample=do_sample)
        e = eos if do_sample else int(base[2])
        tok, _ = _run(view, o, 0, do_sample=do_sample, unfinished=flags, eos_id=e)
        assert tok[1] == PAD_ID and tok[4] == PAD_ID
        assert tok[[0, 2, 3]].tolist() == base[[0, 2, 3]].tolist()
        assert flags.cpu().tolist() == [0 if int(base[0]) == e else 1, 0, 0, 0 if int(base[3]) == e else 1, 0]


def test_min_length_and_uniform_row_follow_the_device_step():
    """The suppress applies while the DEVICE step index is below min_len, and the uniform comes from that step's row of the table."""
    V = 1000
    x, o, q32, _ = _spec(V, "k50")
    view = _strided(x, 3)
    top = int(x[0].float().argmax())
    o1 = dict(top_k=1, suppress_id=top)
    assert int(_run(view, o1, 2, min_len=3)[0][0]) != top and int(_run(view, o1, 3, min_len=3)[0][0]) == top
    uni = torch.tensor([[0.0] * sc.ROWS, [0.999] * sc.ROWS, [0.0] * sc.ROWS], device="cuda")
    a, b = _run(view, o, 0, uniforms=uni)[0], _run(view, o, 1, uniforms=uni)[0]
    assert a.tolist() == _run(view, o, 2, uniforms=uni)[0].tolist() and a.tolist() != b.tolist()


def test_determinism():
    for V, name in ((32274, "p09"), (4099, "t07")):
        x, o, _, _ = _spec(V, name)
        view = _strided(x[torch.arange(64) % sc.ROWS], 3)
        uni = torch.rand(1, 64, generator=torch.Generator().manual_seed(1)).cuda()
        t1, p1 = _run(view, o, 0, uniforms=uni, probs=True)
        t2, p2 = _run(view, o, 0, uniforms=uni, probs=True)
        assert torch.equal(t1, t2) and torch.equal(p1.view(torch.int32), p2.view(torch.int32))


def test_vocabulary_bound():
    """The bound itself (40 000: the whole of the CU's LDS) runs and meets the spec; one above it answers -22 and writes nothing."""
    import ctypes as C
    from emu_amd import _lib, ops
    V = _lib.SAMPLE_MAX_VOCAB
    assert V >= 40000
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(2, V + 1, generator=g) * 3).to(torch.bfloat16)
    o = dict(top_k=50, temperature=0.7)
    tok, pr = _run(_strided(x[:, :V].contiguous(), 3), o, 0, probs=True)
    q64 = sampling.reference_probs(x[:, :V], dtype=torch.float64, **o)
    assert torch.equal(pr > 0, q64 > 0) and float((pr.double() - q64).abs().max()) <= 1e-5
    xd = x.cuda()
    out = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    pr = torch.full((2, V + 1), -1.0, device="cuda")
    flags = torch.ones(2, dtype=torch.int32, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    uni = torch.zeros(1, 2, device="cuda")
    rc = _lib.lib().emu_sample_bf16(xd.data_ptr(), V + 1, 2, V + 1, None, 0, 0, step.data_ptr(), uni.data_ptr(), 2, 1,
                                    C.byref(_params(o)), flags.data_ptr(), out.data_ptr(), pr.data_ptr(), V + 1, ops.stream(xd))
    torch.cuda.synchronize()
    assert rc == -22
    assert out.cpu().tolist() == [-7, -7] and bool((pr == -1.0).all()) and flags.cpu().tolist() == [1, 1]
