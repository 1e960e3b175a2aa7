"""Float64 model of the decoder arithmetic, one layer at a time (test yardstick; plain torch, never
imports the library; runs on whichever device its inputs live on).

The kernels document what they compute (include/pnr.h PNR_PREC_*, csrc/mlp16.h mfma_frag): per layer,
every fp32 operand is split by round-to-nearest-even into 16-bit parts x = hi + lo, hi = r16(x),
lo = r16(x - hi), and W x is the three products Wl xh + Wh xl + Wh xh accumulated in fp32 ('bf16x3' in
bf16 parts, 'f16x3' in f16 parts under the packer's power-of-two weight scale); 'bf16' is the one
product Wh xh, 'fp32' the product of the exact operands.  Evaluated in float64 on the kernel's OWN
saved input of the layer (teacher forcing), that definition differs from a correct kernel by the fp32
accumulation order alone, which the project bounds by BOUND_ULPS u M, u = 2^-24, M = sum |terms| + |b|
the summation magnitude of the element (RELU_ULPS in tests/test_gpu_points_forced.py, MAG_ULPS in
tests/test_gpu_points.py).  A kernel that loses one of the three terms, rounds a part the wrong way or
applies a wrong scale leaves that bound by one to three orders of magnitude (tests/test_split_model.py
shows it on the model itself).

Layer 0 has no saved input in the split precisions (the Fourier features e = sin(x B) are not stored:
csrc/capi.cpp carve_save), so its model forms e in float64 from the kernel's fp32 argument and carries
the kernel's stated sine error de through the layer (`layer0`): e enters the product through its
16-bit parts, so where [e - de, e + de] holds a rounding boundary of a part the operand is uncertain by
one unit of that part, not by de -- `part_spread` evaluates the parts at both ends of the interval.

`backward` forms the float64 gradients from the saved activations and the kernel's own ReLU bits, with
M = sum_p |terms| per element of a parameter gradient (|delta|^T |h| for a weight, sum |delta| for a
bias), the yardstick of tests/test_gpu_points.py strict_bound.  That bound (rtol 1e-3) is too coarse to
see a lost split term of the backward GEMMs -- a known limit; what it adds over the end-to-end tests is
every element, no flip allowance, the bias columns on their own, every precision's save area and ragged
sizes.  dL/dx and dL/dc are not sums over points: their only sum is the delta chain itself, so their M
is the chain's own magnitude (the same chain with |W|, |g| in place of W, g).
"""
import math

import torch

U32 = 2.0 ** -24
BOUND_ULPS = 64.0          # the project's summation bound, in units of u M
EDGE_CAP = 1e-3            # largest share of ReLU pre-activations inside the bound of zero, per layer
DELTA_SC = 6.7e-8          # stated max abs error of fourier_sc (csrc/dev_common.h)
PRECISIONS = ('fp32', 'bf16', 'bf16x3', 'f16x3')
N_FOURIER, N_FOURIER_PAD, HIDDEN, C_DIM = 93, 96, 256, 32
_FMT = {'bf16': torch.bfloat16, 'bf16x3': torch.bfloat16, 'f16x3': torch.float16}


def parts(x32, prec):
    """The operand parts of fp32 values as float64 tensors: [x] (fp32), [hi] (bf16), [hi, lo] (bf16x3 in
    bf16, f16x3 in f16); hi = r16(x), lo = r16(x - hi), both round-to-nearest-even (csrc/mlp16.h
    split_quad, csrc/dev_common.h split2; x - hi is exact in fp32)."""
    assert x32.dtype == torch.float32
    if prec == 'fp32':
        return [x32.double()]
    hi = x32.to(_FMT[prec]).float()
    if prec == 'bf16':
        return [hi.double()]
    lo = (x32 - hi).to(_FMT[prec]).float()
    return [hi.double(), lo.double()]


def weight_scale(W):
    """The f16 images' power-of-two scale of a tensor (csrc/adam.h wscale_from_max): s = 2^e, e =
    floor(log2(fp32(2^14 / max|W|))) clamped to [-20, 20]; 2^20 for an all-zero tensor."""
    mx = W.detach().float().abs().max().cpu()
    e = 20
    if float(mx) > 0:
        q = float(torch.tensor(16384.0, dtype=torch.float32) / mx)
        e = max(-20, min(20, math.frexp(q)[1] - 1))
    return 2.0 ** e


def row_scale(c):
    """Per-row power of two under which the f16x3 feature-branch forward splits the features (csrc/mlp16.h
    fwd16_tile, csrc/dev_common.h pt_scale): uniform over a wave's 32 consecutive rows [32 i, 32 i + 32),
    s = 2^(14 - ex) with max|c| = f 2^ex, f in [0.5, 1), over the wave's rows (rows past P count as 0);
    1 for an all-zero wave; the exponent clamped to [-100, 100].  Returns (P, 1) float32."""
    P = c.shape[0]
    m = torch.zeros(-(-P // 32) * 32, dtype=torch.float32, device=c.device)
    m[:P] = c.detach().float().abs().amax(1)
    m = m.view(-1, 32).amax(1)
    ex = torch.frexp(m)[1]
    s = torch.ldexp(torch.ones_like(m), (14 - ex).clamp(-100, 100))
    s = torch.where(m > 0, s, torch.ones_like(m))
    return s.repeat_interleave(32)[:P, None]


def layer(W, b, h_in, prec, scale=None, inv=None, in_scale=None, terms=None, split=parts):
    """One linear layer z = W h + b on split operands: returns (z, M), float64 (P, out); M = sum over the
    part products of |A| |B| + |b|.  The products are those of mfma_frag (csrc/mlp16.h): Wl xh, Wh xl,
    Wh xh for the split precisions, Wh xh for bf16, W x for fp32.  f16x3: the weights are split as W s,
    s = weight_scale(W), and the accumulator is scaled back by 1 / s.  in_scale: per-row power of two of
    the input (the feature branch: row_scale), undone the same way.
    scale / inv / terms / split exist for the mutants of tests/test_split_model.py: another weight scale,
    an inverse that does not match it, a subset of the three products, another splitting rule."""
    W, h_in = W.detach().float(), h_in.detach().float()
    s = (weight_scale(W) if prec == 'f16x3' else 1.0) if scale is None else scale
    inv = 1.0 / s if inv is None else inv
    x = h_in if in_scale is None else h_in * in_scale
    Wp, xp = split(W * s, prec), split(x, prec)
    prods = [(Wp[1], xp[0]), (Wp[0], xp[1]), (Wp[0], xp[0])] if len(Wp) == 2 else [(Wp[0], xp[0])]
    if terms is not None:
        prods = [prods[i] for i in terms]
    z = sum(xb @ wa.t() for wa, xb in prods)
    M = sum(xb.abs() @ wa.abs().t() for wa, xb in prods)
    if in_scale is not None:
        inv = inv / in_scale.double()
    bd = b.detach().double()
    return z * inv + bd, M * inv + bd.abs()


def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def fourier(x, B):
    """The kernels' Fourier argument x0 B0, fma(x1, B1, .), fma(x2, B2, .) in fp32 (csrc/mlp16.h fwd16_tile,
    csrc/mlp.hip fourier_arg), its float64 sine and the per-feature uncertainty of the kernel's fp32 sine:
    de = 6.7e-8 (fourier_sc's stated error; OCML sinf of the fp32 path is inside it) + 2 u max(1, |arg|)
    for the argument's rounding.  Returns (arg fp32, e float64, de float64), each (P, 93)."""
    x, B = x.detach().float(), B.detach().float()
    arg = (x[:, 0:1].double() * B[0].double()).float()
    arg = _fma32(x[:, 1:2], B[1], arg)
    arg = _fma32(x[:, 2:3], B[2], arg)
    e = torch.sin(arg.double())
    de = DELTA_SC + 2 * U32 * arg.double().abs().clamp(min=1.0)
    return arg, e, de


def part_spread(e, de, prec):
    """How far the parts of the kernel's fp32 e_k in [e - de, e + de] may lie from the parts of fp32(e):
    (uS, uH) = the largest deviation of hi + lo and of hi alone (float64, >= de; both parts are monotone
    in the value, so the ends of the interval decide)."""
    mid = parts(e.float(), prec)
    inf = torch.full_like(e, float('inf')).float()
    uS, uH = de.clone(), de.clone()
    for end in (torch.nextafter((e - de).float(), -inf), torch.nextafter((e + de).float(), inf)):
        p = parts(end, prec)
        uS = torch.maximum(uS, (sum(p) - sum(mid)).abs())
        uH = torch.maximum(uH, (p[0] - mid[0]).abs())
    return uS, uH


def layer0(W0, b0, x, B, prec):
    """Layer 0 of the split precisions, which save no e: (z, M, T) with z, M = layer(W0, b0, fp32(sin), .)
    and T = sum_j (|Wh_kj| uS_j + |Wl_kj| uH_j) / s >= sum_j |W0_kj| de_j the operand uncertainty (module
    docstring), so the kernel's pre-activation lies within BOUND_ULPS u M + T of z."""
    _, e, de = fourier(x, B)
    z, M = layer(W0, b0, e.float(), prec)
    s = weight_scale(W0) if prec == 'f16x3' else 1.0
    Wp = parts(W0.detach().float() * s, prec)
    uS, uH = part_spread(e, de, prec)
    T = uS @ Wp[0].abs().t() if len(Wp) == 1 else uS @ Wp[0].abs().t() + uH @ Wp[1].abs().t()
    return z, M, T / s


def output(Wo, bo, h4, prec, feature_branch):
    """The output layer (z, M).  The feature-branch kernels and the f16x3 forward (k_mlp_fwd16w) run it as
    eight more MFMA steps on split operands under Wo's scale (csrc/mlp16.h fwd16_tile, csrc/mlp16w.h
    out_tile); the bf16 / bf16x3 kernels without features as fp32 FMAs on the unsplit h4 (csrc/mlp16.h
    out_layer), the fp32 kernel on exact operands."""
    return layer(Wo, bo, h4, prec if (feature_branch or prec == 'f16x3') else 'fp32')


def feature_term(Wc, bc, c, prec):
    """f_l = Wc_l c + bc_l of the feature branch (z, M); f16x3 splits c under row_scale."""
    return layer(Wc, bc, c, prec, in_scale=row_scale(c) if prec == 'f16x3' else None)


def forward(params, x, prec, c=None):
    """The whole model chained on its own fp32-rounded activations (what the CPU tests look at; the GPU
    test feeds each layer the kernel's saved input instead).  Returns a list of per-layer dicts
    {z, M, T, f, Mf, h} for the four hidden layers and (raw, M_out)."""
    out, h = [], None
    for li in range(4):
        W, b = params[f'pts_linears.{li}.weight'], params[f'pts_linears.{li}.bias']
        if li == 0:
            z, M, T = layer0(W, b, x, params['embedder._B'], prec)
            if prec == 'fp32':
                T = torch.zeros_like(T)
        else:
            (z, M), T = layer(W, b, h, prec), None
        f = Mf = None
        hv = torch.relu(z)
        if c is not None:
            f, Mf = feature_term(params[f'fc_c.{li}.weight'], params[f'fc_c.{li}.bias'], c, prec)
            hv = hv + f
        h = hv.float()
        out.append(dict(z=z, M=M, T=T, f=f, Mf=Mf, h=h))
    return out, output(params['output_linear.weight'], params['output_linear.bias'], h, prec, c is not None)


def edge_share(z, M, T=None):
    """Share of pre-activations whose sign the bound does not decide: |z| <= BOUND_ULPS u M (+ T)."""
    tol = BOUND_ULPS * U32 * M + (0 if T is None else T)
    return float((z.abs() <= tol).double().mean())


def room_points(bound, P, seed=0):
    """P float32 points drawn uniformly strictly inside `bound` (3, 2): the inputs of
    tests/test_gpu_decoder_layers.py, so that tests/test_split_model.py can look at the same ones."""
    g = torch.Generator().manual_seed(7919 * seed + P)
    b = torch.as_tensor(bound, dtype=torch.float64)
    u = torch.rand((P, 3), generator=g, dtype=torch.float64) * 0.998 + 0.001
    return (b[:, 0] + (b[:, 1] - b[:, 0]) * u).float().contiguous()


def room_features(P, seed=0):
    """(P, 32) float32 point features ~ N(0, 0.1)."""
    g = torch.Generator().manual_seed(104729 * seed + P + 1)
    return (torch.randn((P, C_DIM), generator=g, dtype=torch.float64) * 0.1).float().contiguous()


# ---- the training save area -------------------------------------------------------------------
def decode_save(ws, P):
    """Views of a training workspace (uint8 tensor, pnr_mlp_train_workspace_bytes(P)) in the layout of
    csrc/capi.cpp carve_save, ld = P padded to 128: e [ld][96], h [4][ld][256], x [ld] float4 (x0, x1, x2,
    inside), all fp32, then the ReLU mask words [4][ld / 32][64 lanes] uint4.  Unit u of a point sits in
    lane half (u >> 2) & 1 of its 32-point group, word u >> 6, bit 16 ((u >> 5) & 1) + 4 ((u >> 3) & 3) +
    (u & 3) (csrc/mlp16.h conv1, csrc/mlp.hip save_mask; csrc/mlp16w.h conv1 writes the same words from
    16-point waves).  'masks' is decoded to a bool (4, ld, 256)."""
    ld = -(-P // 128) * 128
    o_h = N_FOURIER_PAD * 4 * ld
    o_x = o_h + 4 * HIDDEN * 4 * ld
    o_m = o_x + 16 * ld
    assert ws.dtype == torch.uint8 and ws.numel() >= o_m + 128 * ld
    words = ws[o_m:o_m + 128 * ld].view(torch.int32).view(4, ld // 32, 2, 32, 4)  # [layer][group][hh][point][word]
    bits = (words.unsqueeze(-1) >> torch.arange(32, dtype=torch.int32, device=ws.device)) & 1
    u = torch.arange(HIDDEN, device=ws.device)
    hh, wi, bit = (u >> 2) & 1, u >> 6, 16 * ((u >> 5) & 1) + 4 * ((u >> 3) & 3) + (u & 3)
    masks = bits.permute(0, 1, 3, 2, 4, 5).reshape(4, ld, 2 * 4 * 32)[:, :, hh * 128 + wi * 32 + bit].bool()
    return dict(ld=ld,
                e=ws[:o_h].view(torch.float32).view(ld, N_FOURIER_PAD),
                h=ws[o_h:o_x].view(torch.float32).view(4, ld, HIDDEN),
                x=ws[o_x:o_m].view(torch.float32).view(ld, 4),
                masks=masks)


# ---- backward ---------------------------------------------------------------------------------
def backward(params, x, h, masks, g_raw, c=None, last_sum=None):
    """Float64 gradients of sum(raw * g_raw) from saved activations: x (P, 3) the fp32 inputs, h the four
    saved (P, 256) activations h1..h4, masks bool (4, P, 256) the ReLU bits [z_l > 0], c (P, 32) the
    features of the feature-branch decoder (params then holds fc_c.*).  Returns {name: (g, M)} for every
    parameter, 'x' (dL/dx) and, with c, 'c' (dL/dc); M as in the module docstring."""
    d = lambda t: t.detach().double()  # noqa: E731
    g = d(g_raw)
    h = [d(t) for t in h]
    arg, e, _ = fourier(x, params['embedder._B'])
    out = {'output_linear.weight': (g.t() @ h[3], g.abs().t() @ h[3].abs()),
           'output_linear.bias': (g.sum(0), g.abs().sum(0))}
    Wo = d(params['output_linear.weight'])
    dh, dhM = g @ Wo, g.abs() @ Wo.abs()
    gc = gcM = gcL = None
    for li in range(3, -1, -1):
        if c is not None:
            cd, Wc = d(c), d(params[f'fc_c.{li}.weight'])
            out[f'fc_c.{li}.weight'] = (dh.t() @ cd, dh.abs().t() @ cd.abs())
            out[f'fc_c.{li}.bias'] = (dh.sum(0), dh.abs().sum(0))
            gc = dh @ Wc if gc is None else gc + dh @ Wc
            gcM = dhM @ Wc.abs() if gcM is None else gcM + dhM @ Wc.abs()
            gcL = dh.abs() @ Wc.abs() if gcL is None else gcL + dh.abs() @ Wc.abs()
        m = masks[li].to(dh.dtype)
        delta, deltaM = dh * m, dhM * m
        inp = h[li - 1] if li > 0 else e
        W = d(params[f'pts_linears.{li}.weight'])
        out[f'pts_linears.{li}.weight'] = (delta.t() @ inp, delta.abs().t() @ inp.abs())
        out[f'pts_linears.{li}.bias'] = (delta.sum(0), delta.abs().sum(0))
        dh, dhM = delta @ W, deltaM @ W.abs()
    cs = torch.cos(arg.double())
    garg, gargM = dh * cs, dhM * cs.abs()
    xd, B = d(x), d(params['embedder._B'])
    out['embedder._B'] = (xd.t() @ garg, xd.abs().t() @ garg.abs())
    out['x'] = (garg @ B.t(), gargM @ B.abs().t())
    last = {'x': garg.abs() @ B.abs().t()}
    if c is not None:
        out['c'] = (gc, gcM)
        last['c'] = gcL
    if last_sum is not None:  # the magnitude of the last sum alone (a printed figure of the GPU test)
        last_sum.update(last)
    return out


def grad_bound(g, M, rtol=1e-3, atol=1e-6):
    """tests/test_gpu_points.py strict_bound with d32 = 0: rtol |g| + atol max|g| + BOUND_ULPS u M."""
    return rtol * g.abs() + atol * g.abs().max().clamp(min=1e-30) + BOUND_ULPS * U32 * M
