"""The CLAP tower's front-end and glue kernels one by one, each against a float64 reference on the CPU
(tests/clap_ops_ref.py), element by element: `ctta_wav_to_logmel_db[_bwd]`, `ctta_htsat_image[_bwd]`,
`ctta_attention_fullbias[_bwd_inplace]`, `ctta_gather_rows`, `ctta_gelu[_bwd]`, `ctta_mean_tokens[_bwd]`,
`ctta_resample_poly[_bwd]`.  The tower tests (tests/test_clap_gpu.py) hold whole-model outputs to a few percent; a wrong
halo term of the STFT adjoint, a wrong bias batch or a wrong fold row stays below that.

Bounds: tests/clap_ops_ref.py states each one and where it comes from; every test prints the figure it measured before
it asserts (LABNOTES.md section XVI records them).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import cases  # noqa: E402
import clap_ops_ref as R  # noqa: E402
from consistencytta_amd import _native as N  # noqa: E402
from consistencytta_amd import clap as C  # noqa: E402
from gpu_util import DEV, bf16_round, det, rel_err, rel_l2, sync  # noqa: E402
from oracle import clap as oclap  # noqa: E402

POISON = 776.0           # exactly representable in bf16 and fp32, outside every value a kernel here produces


def lib():
    return N.lib()


def worst_rel(got, ref, what):
    """max |got - ref| / max |ref|, printed."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    e = float((got - ref).abs().max() / ref.abs().max())
    print("%s: worst |err| / max|ref| = %.3e" % (what, e))
    return e


def assert_bf16_close(got, ref, what, abs_rel=1e-6):
    """|got - ref| <= 2^-8 |ref| + abs_rel * max |ref|: one bf16 rounding of the element plus an absolute term."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    err = (got - ref).abs()
    over = (err - ref.abs() * 2.0 ** -8) / float(ref.abs().max())
    print("%s: worst (|err| - 2^-8 |ref|) / max|ref| = %.3e (allowed %.1e)" % (what, float(over.max()), abs_rel))
    assert float(over.max()) <= abs_rel, (what, int(over.argmax()))


# ------------------------------------------------------------------------------------------------ 1, 2: log-mel
class MelHandle:
    def __init__(self, max_batch=R.LOGMEL_MAX_BATCH, max_samples=R.LOGMEL_MAX_SAMPLES):
        c = R.FRONT_CFG
        self.h = N.c_void_p()
        N.check(lib().ctta_mel_frontend_create(c["n_fft"], c["hop"], c["n_fft"], c["mel_bins"], c["sample_rate"],
                                               float(c["fmin"]), float(c["fmax"]), max_batch, max_samples, self.h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        sync()
        lib().ctta_mel_frontend_destroy(self.h)

    def forward(self, wav):
        B, L = wav.shape
        assert B <= R.LOGMEL_MAX_BATCH and 512 < L <= R.LOGMEL_MAX_SAMPLES
        wd = wav.to(torch.float32).contiguous().to(DEV)
        lm = torch.full((B, L // R.FRONT_CFG["hop"] + 1, R.FRONT_CFG["mel_bins"]), POISON, dtype=torch.float32, device=DEV)
        N.check(lib().ctta_wav_to_logmel_db(self.h, N.ptr(wd), B, L, R.AMIN, N.ptr(lm), N.stream_ptr()))
        sync()
        return lm.cpu()

    def backward(self, dlm, L):
        B = dlm.shape[0]
        assert tuple(dlm.shape) == (B, L // R.FRONT_CFG["hop"] + 1, R.FRONT_CFG["mel_bins"])
        dd = dlm.to(torch.float32).contiguous().to(DEV)
        dwav = torch.full((B, L), POISON, dtype=torch.float32, device=DEV)
        N.check(lib().ctta_wav_to_logmel_db_bwd(self.h, N.ptr(dd), B, L, R.AMIN, N.ptr(dwav), N.stream_ptr()))
        sync()
        return dwav.cpu()


def _dlogmel(L):
    return R.det64("clapops.dlm.%d" % L, (2, L // R.FRONT_CFG["hop"] + 1, R.FRONT_CFG["mel_bins"]), 12).to(torch.float32)


@pytest.mark.parametrize("L", R.LOGMEL_LENGTHS)
def test_wav_to_logmel_db_forward(L):
    """fp32-grade dB values: a lost split pass (-96 dB floor) must show (tests/test_clap_ops_cpu.py has its cost)."""
    wav = R.logmel_inputs(L)
    ref = R.logmel_db_ref(wav)
    mel = R.mel_power64(wav, R.FRONT_CFG)
    assert not bool(((mel > 0) & (mel < 1e-6)).any())          # each value is the exact floor or far above amin
    with MelHandle() as h:
        got = h.forward(wav).double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    floor = got[mel == 0]
    if floor.numel():                                            # silent frames: one value, the kernel's fp32 floor
        print("logmel fwd L=%d: floor %.9f on %d silent entries" % (L, float(floor[0]), floor.numel()))
        assert bool((floor == floor[0]).all())
    err = float((got - ref).abs().max())
    print("logmel fwd L=%d: worst %.3e dB (bound %.1e)" % (L, err, R.LOGMEL_FWD_DB))
    assert err <= R.LOGMEL_FWD_DB


@pytest.mark.parametrize("L", R.LOGMEL_LENGTHS)
def test_wav_to_logmel_db_backward(L):
    wav, dlm = R.logmel_inputs(L), _dlogmel(L)
    rounded = R.logmel_db_bwd_rounded_ref(wav, dlm)
    plain = R.logmel_db_bwd_ref(wav, dlm)
    sil = R.silent_frames(wav)
    with MelHandle() as h:
        h.forward(wav)
        got = h.backward(dlm, L).double()
        got0 = None
        if bool(sil.any()):                                      # silent frames must contribute exactly nothing
            dlm0 = dlm.clone()
            dlm0[sil] = 0.0
            got0 = h.backward(dlm0, L).double()
    e_r = worst_rel(got, rounded, "logmel bwd L=%d vs rounded ref" % L)
    e_p = worst_rel(got, plain, "logmel bwd L=%d vs plain float64" % L)
    halo = R.halo_mask(L)
    h_r = worst_rel(got[:, halo], rounded[:, halo], "logmel bwd L=%d halo vs rounded ref" % L)
    h_p = worst_rel(got[:, halo], plain[:, halo], "logmel bwd L=%d halo vs plain float64" % L)
    assert e_r <= R.LOGMEL_BWD_ROUNDED and h_r <= R.LOGMEL_BWD_ROUNDED
    assert e_p <= R.LOGMEL_BWD_PLAIN and h_p <= R.LOGMEL_BWD_PLAIN
    assert (got0 is not None) == (L >= 2400)
    if got0 is not None:
        assert torch.equal(got0, got)


def test_logmel_backward_uses_the_latest_forward():
    """Two forwards on one handle, then a backward: bit-equal to a fresh handle that only saw the second waveform."""
    L = 1447
    first, second, dlm = R.logmel_inputs(4801)[:, :L].contiguous(), R.logmel_inputs(L), _dlogmel(L)
    with MelHandle() as a, MelHandle() as b:
        a.forward(first)
        lm_a = a.forward(second)
        da = a.backward(dlm, L)
        lm_b = b.forward(second)
        db = b.backward(dlm, L)
    assert torch.equal(lm_a, lm_b) and torch.equal(da, db)
    assert float(da.abs().max()) > 0 and not torch.equal(first, second)


# ------------------------------------------------------------------------------------------------ 3: image
def _tap_tables(frames, tt):
    fe = C._FrontendState(dict(R.FRONT_CFG, spec_size=64, patch_size=4))
    return fe.tap_tables(frames, tt, DEV)


@pytest.mark.parametrize("S,Fq,ps,frames", R.IMAGE_GEOMETRIES)
def test_htsat_image_forward_and_backward(S, Fq, ps, frames):
    B, cpad = 2, 8
    tt = S * (S // Fq)
    lm, scale, shift = R.image_inputs(S, Fq, ps, frames, B)
    ref = R.image_ref(lm, scale, shift, S)
    tabs = _tap_tables(frames, tt)
    lmd, sd_, cd = lm.to(DEV), scale.to(DEV), shift.to(DEV)
    img = torch.full((B, S, S, cpad), POISON, dtype=torch.bfloat16, device=DEV)
    N.check(lib().ctta_htsat_image(N.ptr(lmd), B, frames, Fq, N.ptr(sd_), N.ptr(cd), N.ptr(tabs["idx"]), N.ptr(tabs["w"]),
                                   tt, S, cpad, N.ptr(img), N.stream_ptr()))
    sync()
    img = img.float().cpu()
    assert float(img[..., 1:].abs().max()) == 0.0                # pad channels
    assert_bf16_close(img[..., 0], ref, "image fwd %s" % ((S, Fq, ps, frames),))
    G = S // ps
    for ld in (ps * ps, 64):
        dtok = R.det64("clapops.img.dtok.%d.%d" % (S, frames), (B, G * G, ld), 4).to(torch.float32)
        dref = R.image_bwd_ref(lm, scale, shift, S, ps, dtok)
        dlm = torch.full((B, frames, Fq), POISON, dtype=torch.float32, device=DEV)
        dtd = dtok.contiguous().to(DEV)
        N.check(lib().ctta_htsat_image_bwd(N.ptr(dtd), ld, ps, B, frames, Fq, N.ptr(sd_), N.ptr(tabs["rt_ptr"]),
                                           N.ptr(tabs["rt_tt"]), N.ptr(tabs["rt_w"]), S, N.ptr(dlm), N.stream_ptr()))
        sync()
        e = worst_rel(dlm, dref, "image bwd %s ld=%d" % ((S, Fq, ps, frames), ld))
        e_t = worst_rel(dlm, R.image_bwd_ref(lm, scale, shift, S, ps, dtok, host_taps=True),
                        "image bwd %s ld=%d vs host taps" % ((S, Fq, ps, frames), ld))
        assert e <= R.IMAGE_BWD and e_t <= R.IMAGE_BWD_TAPS


# ------------------------------------------------------------------------------------------------ 4: _Frontend
@pytest.mark.parametrize("L", [9000, 28800])
def test_frontend_input_gradient_against_oracle(L):
    """d (tok * g).sum() / d wav through `_Frontend` (patch-embedding data gradient, image, log-mel and STFT adjoints)
    against the oracle's `wav_to_image` + conv2d under autograd."""
    cfg = cases.TINY_HTSAT
    m = C.HTSAT(cfg)
    gold = np.load(cases.__file__.replace("cases.py", "clap_htsat.npz"))
    sd = cases.clap_weights(gold["tiny_keys"], gold["tiny_shapes"], "tiny", 5)
    m.load_state_dict(sd, strict=False)
    m.to(DEV)
    B, G, Cc = 2, cfg["spec_size"] // cfg["patch_size"], cfg["embed_dim"]
    wav = (det("fe.wav", (B, L), 7) * 0.4).requires_grad_(True)
    g = bf16_round(det("clapops.fe.g", (B, G, G, Cc), 3))
    tref = F.conv2d(oclap.wav_to_image(cfg, sd, wav, prefix=""), bf16_round(sd["patch_embed.proj.weight"]),
                    sd["patch_embed.proj.bias"], stride=cfg["patch_stride"])
    (tref * g.permute(0, 3, 1, 2)).sum().backward()
    P = m._pack()
    wd = wav.detach().to(DEV).requires_grad_(True)
    tok = C._Frontend.apply(wd, m._fe, P["patch"], P["patch_t"])
    assert tuple(tok.shape) == (B * G * G, Cc)
    (tok.float() * g.reshape(B * G * G, Cc).to(DEV)).sum().backward()
    sync()
    got, ref = wd.grad.cpu(), wav.grad
    e = rel_l2(got, ref)
    print("frontend grad L=%d: rel_l2 %.3e (bound %.1e)" % (L, e, R.FRONTEND_GRAD_REL_L2))
    assert float(ref.abs().max()) > 0
    assert e <= R.FRONTEND_GRAD_REL_L2
    if L == 9000:
        halo = R.halo_mask(L)
        assert worst_rel(got[:, halo], ref[:, halo], "frontend grad L=%d halo" % L) <= R.FRONTEND_GRAD_HALO


# ------------------------------------------------------------------------------------------------ 5: window attention
def _pad_heads(x, heads, hd):
    """(nw, heads, n, hd) -> [nw * n][heads * 64] with each head in its own 64-lane block."""
    nw, _, n, _ = x.shape
    out = torch.zeros(nw * n, heads, 64, dtype=torch.float64)
    out[:, :, :hd] = x.permute(0, 2, 1, 3).reshape(nw * n, heads, hd)
    return out.reshape(nw * n, heads * 64)


def _unpad_heads(x, nw, n, heads, hd):
    x = x.detach().double().cpu().contiguous().view(nw, n, heads, 64)
    return x[..., :hd].permute(0, 2, 1, 3), x[..., hd:]


@pytest.mark.parametrize("heads,hd,n,nw,nbb", R.ATTN_CASES)
def test_window_attention_fullbias_per_element(heads, hd, n, nw, nbb):
    q, k, v, go, bias, dead = R.attention_inputs(heads, hd, n, nw, nbb)
    scale = hd ** -0.5
    o_ref, lse_ref = R.window_attention_ref(q, k, v, bias, scale)
    grads_ref = R.window_attention_bwd_ref(q, k, v, bias, scale, go)
    hp = heads * 64
    qkv = torch.cat([_pad_heads(t, heads, hd) for t in (q, k, v)], 1).to(torch.bfloat16).to(DEV)
    junk = torch.full((nw * n, 3 * hp), POISON, dtype=torch.bfloat16, device=DEV)       # what fresh buffers may hold
    del junk
    qd = qkv.requires_grad_(True)
    bias_log2 = (bias.to(torch.float32) * C.LOG2E).contiguous().to(DEV)
    out = C._WindowAttention.apply(qd, bias_log2, nbb, heads, n, scale)
    sync()
    tag = "attn %s" % ((heads, hd, n, nw, nbb),)
    got, pad = _unpad_heads(out, nw, n, heads, hd)
    assert float(pad.abs().max()) == 0.0
    assert_bf16_close(got, o_ref, tag + " out", R.ATTN_FWD_ABS)
    lse = next(t for t in out.grad_fn.saved_tensors if t.dtype == torch.float32 and tuple(t.shape) == (nw, heads, n))
    e_lse = float((lse.double().cpu() - lse_ref).abs().max())
    print("%s lse: worst abs %.3e (bound %.1e)" % (tag, e_lse, R.ATTN_LSE_ABS))
    assert e_lse <= R.ATTN_LSE_ABS
    out.backward(_pad_heads(go, heads, hd).to(torch.bfloat16).to(DEV))
    sync()
    dqkv = qd.grad
    for part, (name, ref) in enumerate(zip(("dq", "dk", "dv"), grads_ref)):
        got, pad = _unpad_heads(dqkv[:, part * hp:(part + 1) * hp], nw, n, heads, hd)
        assert float(pad.abs().max()) == 0.0, name
        e = worst_rel(got, ref, "%s %s" % (tag, name))
        assert e <= R.ATTN_BWD[name], name
        if dead is not None and name != "dq":                    # keys no query can see
            b, k0 = dead
            assert float(ref[b, :, k0:].abs().max()) < 1e-30
            assert float(got[b, :, k0:].abs().max()) <= R.ATTN_BWD[name] * float(ref.abs().max()), name


@pytest.mark.parametrize("heads,hd,n,nw,nbb", [(2, 32, 12, 5, 2),     # vt_ld = 16: a 16-byte vector of V^T straddles nk
                                               (3, 16, 20, 4, 4)])    # vt_ld = 24
def test_fullbias_bwd_inplace_reads_no_vt_column_beyond_the_keys(heads, hd, n, nw, nbb):
    """`ctta_attention_fullbias_bwd_inplace` through the C ABI where n is no multiple of 8: the V^T columns >= n are NaN."""
    q, k, v, go, bias, _ = R.attention_inputs(heads, hd, n, nw, nbb)
    scale = hd ** -0.5
    grads_ref = R.window_attention_bwd_ref(q, k, v, bias, scale, go)
    L, st, hp, vt_ld = lib(), N.stream_ptr(), heads * 64, (n + 7) // 8 * 8
    qd, kd, vd, dod = (_pad_heads(t, heads, hd).to(torch.bfloat16).to(DEV) for t in (q, k, v, go))
    vt = torch.full((nw, hp, vt_ld), float("nan"), dtype=torch.bfloat16, device=DEV)
    vt[:, :, :n] = vd.view(nw, n, hp).transpose(1, 2)
    bias_log2 = (bias.to(torch.float32) * C.LOG2E).contiguous().to(DEV)
    out = torch.empty(nw * n, hp, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(nw, heads, n, dtype=torch.float32, device=DEV)
    N.check(L.ctta_attention_fullbias(N.ptr(qd), hp, N.ptr(kd), hp, n, N.ptr(vt), vt_ld, N.ptr(bias_log2), nbb, N.ptr(out), hp,
                                      nw, heads, n, n, float(scale), N.ptr(lse), st))
    dsum = torch.empty(nw, heads, n, dtype=torch.float32, device=DEV)
    grads = [torch.full((nw * n, hp), POISON, dtype=torch.bfloat16, device=DEV) for _ in range(3)]
    N.check(L.ctta_attention_fullbias_bwd_inplace(
        N.ptr(qd), hp, N.ptr(kd), hp, n, N.ptr(vt), vt_ld, N.ptr(bias_log2), nbb, N.ptr(out), hp, N.ptr(dod), hp, N.ptr(lse),
        N.ptr(dsum), N.ptr(grads[0]), hp, N.ptr(grads[1]), hp, N.ptr(grads[2]), hp, nw, heads, n, n, float(scale), st))
    sync()
    tag = "attn abi %s" % ((heads, hd, n, nw, nbb),)
    for name, g, ref in zip(("dq", "dk", "dv"), grads, grads_ref):
        got, pad = _unpad_heads(g, nw, n, heads, hd)
        assert float(pad.abs().max()) == 0.0, name
        assert worst_rel(got, ref, "%s %s" % (tag, name)) <= R.ATTN_BWD[name], name     # worst_rel: finite, too


# ------------------------------------------------------------------------------------------------ 6: glue
def _bits(x):
    return x.contiguous().view(torch.int16)


@pytest.mark.parametrize("row_elems,n_src,n_rows", [(8, 41, 97), (64, 41, 97), (200, 41, 97), (8, 1000, 8192 * 256 + 37)])
def test_gather_rows_strides_and_second_trip(row_elems, n_src, n_rows):
    src_ld, dst_ld = row_elems + 8, row_elems + 24
    gen = torch.Generator().manual_seed(row_elems + n_rows)
    src = torch.full((n_src, src_ld), -POISON, dtype=torch.bfloat16)
    src[:, :row_elems] = (torch.rand(n_src, row_elems, generator=gen) * 8 - 4).to(torch.bfloat16)
    idx = torch.randint(0, n_src, (n_rows,), generator=gen, dtype=torch.int32)           # repeated sources
    idx[torch.randint(0, n_rows, (max(3, n_rows // 50),), generator=gen)] = -1
    idx[0], idx[n_rows - 1] = n_src - 1, -1
    assert n_rows > n_src and int((idx == -1).sum()) >= 2
    srcd, idxd = src.to(DEV), idx.to(DEV)
    dst = torch.full((n_rows, dst_ld), POISON, dtype=torch.bfloat16, device=DEV)
    N.check(lib().ctta_gather_rows(N.ptr(srcd), src_ld, N.ptr(idxd), N.ptr(dst), dst_ld, n_rows, row_elems, N.stream_ptr()))
    sync()
    ref = srcd[idxd.clamp(min=0).long(), :row_elems]                                      # torch indexing
    ref = torch.where((idxd >= 0)[:, None], ref, torch.zeros_like(ref))
    assert torch.equal(_bits(dst[:, :row_elems]), _bits(ref))
    assert bool((dst[:, row_elems:] == POISON).all())                                     # padding untouched
    if n_rows * (row_elems // 8) > 8192 * 256:
        assert n_rows * (row_elems // 8) - 8192 * 256 < 256                               # the second trip is one short block
    with pytest.raises(N.CttaError):                                                      # a destination row shorter than the data
        N.check(lib().ctta_gather_rows(N.ptr(srcd), src_ld, N.ptr(idxd), N.ptr(dst), row_elems - 8, n_rows, row_elems,
                                       N.stream_ptr()))


GELU_PATTERN = 2056


def _gelu_inputs(n):
    """bf16 values spanning [-6, 6], with +-0 and +-10 (where the pdf underflows) in front; tiled for the large size."""
    m = min(n, GELU_PATTERN)
    x = torch.linspace(-6.0, 6.0, m, dtype=torch.float64)
    x[:4] = torch.tensor([0.0, -0.0, 10.0, -10.0], dtype=torch.float64)
    x = R.bf16_round64(x)
    dy = R.bf16_round64(R.det64("clapops.gelu.dy", (m,), 2))
    return x, dy


def _tile(t, n):
    reps = n // t.numel()
    return torch.cat([t.repeat(reps), t[:n - reps * t.numel()]])


@pytest.mark.parametrize("n", [8, GELU_PATTERN, 8192 * 256 * 8 + 8])
def test_gelu_forward_backward_per_element(n):
    x, dy = _gelu_inputs(n)
    y_ref, dx_ref = R.gelu64(x), dy * R.gelu_grad64(x)
    assert float(y_ref[2]) == 10.0 and float(y_ref[3].abs()) < 1e-20
    xd, dyd = _tile(x.to(torch.bfloat16).to(DEV), n), _tile(dy.to(torch.bfloat16).to(DEV), n)
    y = torch.full((n,), POISON, dtype=torch.bfloat16, device=DEV)
    dx = torch.full((n,), POISON, dtype=torch.bfloat16, device=DEV)
    N.check(lib().ctta_gelu(N.ptr(xd), N.ptr(y), n, N.stream_ptr()))
    N.check(lib().ctta_gelu_bwd(N.ptr(xd), N.ptr(dyd), N.ptr(dx), n, N.stream_ptr()))
    sync()
    for name, got, ref in (("gelu", y, y_ref), ("gelu_bwd", dx, dx_ref)):
        refd = _tile(ref.to(DEV), n)                              # float64; the comparison itself runs on the device
        over = ((got.double() - refd).abs() - refd.abs() * 2.0 ** -8) / float(ref.abs().max())
        print("%s n=%d: worst (|err| - 2^-8 |ref|) / max|ref| = %.3e (allowed 1e-6)" % (name, n, float(over.max())))
        assert bool(torch.isfinite(got.float()).all())
        assert float(over.max()) <= 1e-6, name


def test_gelu_refuses_a_length_that_is_no_multiple_of_eight():
    x = torch.zeros(16, dtype=torch.bfloat16, device=DEV)
    y = torch.zeros(16, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(N.CttaError):
        N.check(lib().ctta_gelu(N.ptr(x), N.ptr(y), 12, N.stream_ptr()))
    with pytest.raises(N.CttaError):
        N.check(lib().ctta_gelu_bwd(N.ptr(x), N.ptr(x), N.ptr(y), 12, N.stream_ptr()))


@pytest.mark.parametrize("B,tokens,Cc,ld", [(3, 16, 128, 128), (2, 4, 1024, 1024), (2, 7, 300, 320)])
def test_mean_tokens_forward_backward(B, tokens, Cc, ld):
    x = torch.full((B * tokens, ld), -POISON, dtype=torch.float64)
    x[:, :Cc] = R.bf16_round64(R.det64("clapops.mt.x.%d" % Cc, (B * tokens, Cc), 1) * 2.0)
    xd = x.to(torch.bfloat16).to(DEV)
    y = torch.full((B, Cc), POISON, dtype=torch.float32, device=DEV)
    N.check(lib().ctta_mean_tokens(N.ptr(xd), B, tokens, Cc, ld, N.ptr(y), N.stream_ptr()))
    sync()
    ref = x[:, :Cc].view(B, tokens, Cc).mean(1)
    assert rel_err(y, ref) < 1e-6
    dy = R.det64("clapops.mt.dy.%d" % Cc, (B, Cc), 2).to(torch.float32)
    dx = torch.full((B * tokens, ld), POISON, dtype=torch.bfloat16, device=DEV)
    N.check(lib().ctta_mean_tokens_bwd(N.ptr(dy.to(DEV)), B, tokens, Cc, ld, N.ptr(dx), N.stream_ptr()))
    sync()
    want = (dy / torch.tensor(float(tokens), dtype=torch.float32)).to(torch.bfloat16)    # bf16(fp32 dy / tokens)
    want = want[:, None, :].expand(B, tokens, Cc).reshape(B * tokens, Cc)
    dx = dx.cpu()
    assert torch.equal(_bits(dx[:, :Cc]), _bits(want))
    assert bool((dx[:, Cc:] == POISON).all())


@pytest.mark.parametrize("orig,new,L", R.RESAMPLE_CASES)
def test_resampler_adjoint_identity_and_clipped_windows(orig, new, L):
    """<R x, g> = <x, R^T g> with the sums in float64; the two shortest cases are shorter than the filter, so every tap
    window is clipped on both sides."""
    x = det("clapops.rs.x", (2, L), 1) * 0.8
    rs = C.Resampler(orig, new, **R.KAISER)
    if L < 64:
        assert L < rs.kernels.shape[1]
    xd = x.to(DEV).requires_grad_(True)
    y = rs(xd)
    g = det("clapops.rs.g", tuple(y.shape), 2)
    (y * g.to(DEV)).sum().backward()
    sync()
    xr = x.clone().requires_grad_(True)
    ref = oclap.resample(xr, orig, new, **R.KAISER)
    (ref * g).sum().backward()
    assert y.shape == ref.shape
    assert rel_err(y, ref) < 2e-5 and rel_err(xd.grad, xr.grad) < 2e-5
    x64 = x.double().requires_grad_(True)                         # the same filter table, sums in float64
    ref64 = R.resample64(x64, orig, new, **R.KAISER)
    (ref64 * g.double()).sum().backward()
    e_y, e_g = rel_err(y, ref64), rel_err(xd.grad, x64.grad)
    print("resample %s vs float64: y %.3e, dx %.3e" % ((orig, new, L), e_y, e_g))
    assert e_y < 2e-5 and e_g < 2e-5
    yg = y.detach().double().cpu() * g.double()
    lhs, rhs = float(yg.sum()), float((x.double() * xd.grad.double().cpu()).sum())
    print("resample %s: <Rx,g> %.9e  <x,R^T g> %.9e  sum|.| %.3e" % ((orig, new, L), lhs, rhs, float(yg.abs().sum())))
    assert abs(lhs - rhs) <= 1e-6 * float(yg.abs().sum())
