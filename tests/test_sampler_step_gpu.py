"""Op-level parity of the sampler-step kernels (dd_op_sampler_step / dd_op_sampler_step_bwd, include/distdiff_hip_ops.h): the step of
every prediction type and the classifier-free-guidance rescale against the float64 restatement of tests/sampler_variants_ref.py and
float64 autograd of it.

Shapes (B, C, L): (2, 4, 8) the shape of the cfg_ddim test; (3, 4, 6) 36 pixels, ragged against the 256-pixel blocks, odd batch;
(2, 4, 96) 9216 pixels = 36 first-stage blocks per image and a real second stage.  The model output lives in 8-wide fp32 rows with 1e30
in columns 4-7: a kernel that lets padding into a result shows it.
Tolerances: fp32 outputs max|err| <= 1e-5 + 1e-5 max|ref| and the bf16 gradient rows 1e-3 + 1e-2 max|ref| (the figures of
tests/test_kernels_gpu.py::test_elementwise_sampler_ops); the rescale factor 1e-5 relative."""
import ctypes as C

import pytest
import torch

import sampler_variants_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(2, 4, 8), (3, 4, 6), (2, 4, 96)]
S = 7.5
A, AP = 0.64, 0.81


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def close(got, ref, rtol=1e-5, atol=1e-5, what=""):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what + ": non-finite output"
    err, lim = (got - ref).abs().max().item(), atol + rtol * ref.abs().max().item()
    assert err <= lim, "%s: max err %.4g > %.4g (ref max %.4g)" % (what, err, lim, ref.abs().max().item())


@pytest.fixture(scope="module")
def L(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def rows8(x2):
    """[2B, C, H, W] -> fp32 rows [2B*HW, 8] with 1e30 in the padding columns."""
    n, Cc = x2.shape[0] * x2.shape[2] * x2.shape[3], x2.shape[1]
    r = torch.full((n, 8), 1e30)
    r[:, :Cc] = x2.permute(0, 2, 3, 1).reshape(-1, Cc)
    return r


def unrows(g, B2, Cc, Ls):
    return g.float().cpu()[:, :Cc].reshape(B2, Ls, Ls, Cc).permute(0, 3, 1, 2)


def make(shape, seed, offset=False):
    B, Cc, Ls = shape
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, Cc, Ls, Ls, generator=g)
    m2 = torch.randn(2 * B, Cc, Ls, Ls, generator=g)
    if offset:
        m2 = 30.0 + 0.5 * m2
    gx0, gzp = torch.randn(B, Cc, Ls, Ls, generator=g), torch.randn(B, Cc, Ls, Ls, generator=g)
    return z, m2, gx0, gzp


class Step:
    """One (prediction type, a, a', phi) on the device: coefficient rows, scratch, forward and backward calls."""

    def __init__(self, L, pred, shape, a=A, ap=AP, phi=0.0):
        self.L, self.pred, self.code, self.phi, self.a, self.ap = L, pred, R.PRED[pred], phi, a, ap
        self.B, self.Cc, self.Ls = shape
        self.HW = self.Ls * self.Ls
        self.coef = torch.tensor([S, a ** 0.5, (1 - a) ** 0.5, ap ** 0.5, (1 - ap) ** 0.5]).cuda()       # five floats, as cfg_ddim takes
        out = (C.c_float * 4)()
        assert L.dd_op_step_coefs(self.code, a, ap, out) == 0
        self.lin = torch.tensor(list(out)).cuda()
        self.stats = torch.zeros(self.B, 8, device="cuda")
        self.part = torch.zeros(int(L.dd_op_sampler_step_scratch_floats(self.B, self.HW)), device="cuda")

    def fwd(self, z, m2):
        self.d_m2, d_z = rows8(m2).cuda(), z.cuda()
        zp, x0 = torch.empty_like(d_z), torch.empty_like(d_z)
        rc = self.L.dd_op_sampler_step(P(self.d_m2), 8, P(d_z), P(zp), P(x0), self.B, self.Cc, self.HW, P(self.coef), P(self.lin), self.code,
                                       self.phi, P(self.stats), P(self.part), None)
        assert rc == 0
        torch.cuda.synchronize()
        return x0, zp

    def bwd(self, gx0, gzp):
        d_gx0, d_gzp = (gx0.cuda() if gx0 is not None else None), (gzp.cuda() if gzp is not None else None)
        g_m2 = torch.full((2 * self.B * self.HW, 8), 7.0, device="cuda", dtype=torch.bfloat16)
        g_z = torch.empty(self.B, self.Cc, self.Ls, self.Ls, device="cuda")
        rc = self.L.dd_op_sampler_step_bwd(P(d_gx0), P(d_gzp), P(g_m2), 8, P(g_z), self.B, self.Cc, self.HW, P(self.coef), P(self.lin), self.code,
                                           self.phi, P(self.d_m2), P(self.stats), P(self.part), None)
        assert rc == 0
        torch.cuda.synchronize()
        assert float(g_m2[:, self.Cc:].float().abs().max()) == 0.0          # padding columns are written, as zeros
        return g_z, g_m2

    def ref(self, z, m2, gx0=None, gzp=None, grads=False):
        z, m2 = z.double().requires_grad_(grads), m2.double().requires_grad_(grads)
        u, c = m2.chunk(2)
        x0, zp, k = R.cfg_step_ref(self.pred, self.a, self.ap, S, self.phi, z, u, c)
        if not grads:
            return x0.detach(), zp.detach(), k
        outs, cots = [], []
        if gx0 is not None:
            outs.append(x0); cots.append(gx0.double())
        if gzp is not None:
            outs.append(zp); cots.append(gzp.double())
        gz, gm = torch.autograd.grad(outs, [z, m2], cots, allow_unused=True)      # `sample`: x0 = m does not depend on z
        return (gz if gz is not None else torch.zeros_like(z)), gm


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction", "sample"])
def test_step_forward_and_backward(L, pred, shape):
    z, m2, gx0, gzp = make(shape, 8)
    # (epsilon, phi = 0) runs the cfg_ddim kernels behind the same entry points (test_epsilon_mode_is_cfg_ddim_bitwise); the linear
    # form of epsilon is checked with rescale on (test_guidance_rescale)
    st = Step(L, pred, shape)
    x0, zp = st.fwd(z, m2)
    rx0, rzp, _ = st.ref(z, m2)
    close(x0, rx0, what="%s x0" % pred)
    close(zp, rzp, what="%s z_prev" % pred)
    for cx, cz in ((gx0, gzp), (None, gzp), (gx0, None)):
        g_z, g_m2 = st.bwd(cx, cz)
        rgz, rgm = st.ref(z, m2, cx, cz, grads=True)
        close(g_z, rgz, what="%s g_z" % pred)
        close(unrows(g_m2, 2 * shape[0], shape[1], shape[2]), rgm, rtol=1e-2, atol=1e-3, what="%s g_m2" % pred)


def test_v_prediction_at_zero_snr(L):
    """a = 0 exactly (first trailing step of a zero-terminal-SNR table): nothing divides by sqrt(a); x0 = -m."""
    shape = SHAPES[1]
    z, m2, gx0, gzp = make(shape, 9)
    st = Step(L, "v_prediction", shape, a=0.0, ap=0.0047)
    x0, zp = st.fwd(z, m2)
    u, c = m2.double().chunk(2)
    close(x0, -(u + S * (c - u)), what="x0 = -m")
    close(zp, st.ref(z, m2)[1], what="z_prev")
    g_z, g_m2 = st.bwd(gx0, gzp)
    rgz, rgm = st.ref(z, m2, gx0, gzp, grads=True)
    close(g_z, rgz, what="g_z")
    close(unrows(g_m2, 2 * shape[0], shape[1], shape[2]), rgm, rtol=1e-2, atol=1e-3, what="g_m2")


@pytest.mark.parametrize("shape", SHAPES)
def test_epsilon_mode_is_cfg_ddim_bitwise(L, shape):
    """(epsilon, phi = 0) through the new entry points is dd_op_cfg_ddim / dd_op_cfg_ddim_bwd: same bits; lin / stats / part may be NULL."""
    B, Cc, Ls = shape
    HW = Ls * Ls
    z, m2, gx0, gzp = make(shape, 10)
    d_m2, d_z, d_gx0, d_gzp = rows8(m2).cuda(), z.cuda(), gx0.cuda(), gzp.cuda()
    coef = torch.tensor([S, A ** 0.5, (1 - A) ** 0.5, AP ** 0.5, (1 - AP) ** 0.5]).cuda()
    out = [[torch.empty_like(d_z) for _ in range(3)] + [torch.zeros((2 * B * HW, 8), device="cuda", dtype=torch.bfloat16)] for _ in range(2)]
    assert L.dd_op_cfg_ddim(P(d_m2), 8, P(d_z), P(out[0][0]), P(out[0][1]), B, Cc, HW, P(coef), None) == 0
    assert L.dd_op_cfg_ddim_bwd(P(d_gx0), P(d_gzp), P(out[0][3]), 8, P(out[0][2]), B, Cc, HW, P(coef), None) == 0
    assert L.dd_op_sampler_step(P(d_m2), 8, P(d_z), P(out[1][0]), P(out[1][1]), B, Cc, HW, P(coef), None, 0, 0.0, None, None, None) == 0
    assert L.dd_op_sampler_step_bwd(P(d_gx0), P(d_gzp), P(out[1][3]), 8, P(out[1][2]), B, Cc, HW, P(coef), None, 0, 0.0, None, None, None, None) == 0
    torch.cuda.synchronize()
    for a, b in zip(out[0], out[1]):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    # and what is not built is refused in front of any launch: an unknown type, rescale without its buffers, a row stride of 4
    assert L.dd_op_sampler_step(P(d_m2), 8, P(d_z), P(out[1][0]), P(out[1][1]), B, Cc, HW, P(coef), P(coef), 3, 0.0, None, None, None) != 0
    assert L.dd_op_sampler_step(P(d_m2), 8, P(d_z), P(out[1][0]), P(out[1][1]), B, Cc, HW, P(coef), P(coef), 1, 0.5, None, None, None) != 0
    assert L.dd_op_sampler_step(P(d_m2), 4, P(d_z), P(out[1][0]), P(out[1][1]), B, Cc, HW, P(coef), P(coef), 1, 0.0, None, None, None) != 0


@pytest.mark.parametrize("offset", [False, True], ids=["unit", "offset30"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pred", ["v_prediction", "epsilon"])
def test_guidance_rescale(L, pred, shape, offset):
    """phi = 0.7.  offset30: the model output is 30 + 0.5 N(0,1) -- a one-pass sum-of-squares variance in fp32 is wrong in the third digit
    there, the centred two-stage merge is not."""
    phi = 0.7
    z, m2, gx0, gzp = make(shape, 12, offset)
    st = Step(L, pred, shape, phi=phi)
    x0, zp = st.fwd(z, m2)
    rx0, rzp, k = st.ref(z, m2)
    stats = st.stats.cpu().double()
    u, c = m2.double().chunk(2)
    m = u + S * (c - u)
    dims = [1, 2, 3]
    kerr = ((stats[:, 0] - k).abs() / k.abs()).max().item()
    print("rescale factor %s %s %s: k %s, max rel err %.3g" % (pred, shape, "offset" if offset else "unit", k.tolist(), kerr))
    assert kerr <= 1e-5, kerr
    assert ((stats[:, 1] - c.std(dim=dims)).abs() / c.std(dim=dims)).max() <= 1e-5
    assert ((stats[:, 2] - m.std(dim=dims)).abs() / m.std(dim=dims)).max() <= 1e-5
    assert stats[:, 5].tolist() == [float(shape[1] * shape[2] ** 2)] * shape[0]
    close(x0, rx0, what="x0")
    close(zp, rzp, what="z_prev")
    saved = st.stats.clone()
    for cx, cz in ((gx0, gzp), (None, gzp), (gx0, None)):
        g_z, g_m2 = st.bwd(cx, cz)
        rgz, rgm = st.ref(z, m2, cx, cz, grads=True)
        close(g_z, rgz, what="g_z")
        close(unrows(g_m2, 2 * shape[0], shape[1], shape[2]), rgm, rtol=1e-2, atol=1e-3, what="g_m2")
    # no atomics: a second run of the same calls gives the same bits
    g_z, g_m2 = st.bwd(gx0, gzp)
    x0b, zpb = st.fwd(z, m2)
    g_zb, g_m2b = st.bwd(gx0, gzp)
    assert torch.equal(x0, x0b) and torch.equal(zp, zpb) and torch.equal(saved, st.stats) and torch.equal(g_z, g_zb) and torch.equal(g_m2, g_m2b)
