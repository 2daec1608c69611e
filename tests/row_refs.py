"""Float64 references and derived element-wise bounds for the LayerNorm and masked-softmax row kernels (csrc/rowops.hip).

Plain torch on CPU or GPU tensors; nothing of the product is imported.  Every reference is built from the SAME rounded inputs the kernel
reads (a bf16 input is upcast, not regenerated).  With u = 2^-24 (1 + 2^-20):

* a sum of n f32 terms in any order:  |err| <= (n + 2) u sum |term|
* a bf16 result adds half a bf16 ulp taken at |ref| + (f32 bound)

The bounds below are those two rules pushed through each operation; nothing is tuned.  K_RSQRT and K_EXP (ulps of the device rsqrtf /
expf) are the only constants that are not derived.  test_row_refs_cpu.py shows that an honest f32 emulation stays inside every bound and
that the listed mutants do not; test_row_ops_gpu.py holds every kernel form to them.

LayerNorm forward (v = x + x2, n = cols, d = v - mu, s2 = var + eps, h = 1 with x2 else 0):
    D_mu  = (n + 2 + h) u sum|v| / n
    d_d   = D_mu + u |d| + h u |v|
    r_var = (n + 8) u + D_mu^2 / s2 + h 2u sum(|d| |v|) / (n s2)
    r_rs  = r_var / 2 + (K_RSQRT + 1) u
    |dy|  <= |gamma| (rs d_d (1 + r_rs) + |xh| (r_rs + 3u)) + u |y| + u |beta|
    |d mean| <= D_mu + u |mu|,   |d rstd| <= r_rs rstd
LayerNorm backward (the f32 mean / rstd handed to the kernel are exact inputs):
    d_xh  = u |xh| + rs (1 + u) (u |v - mu| + h u |v|)
    d_m1  = (n + 3) u sum|gy| / n
    d_m2  = ((n + 4) u sum|gy xh| + sum|gy| d_xh) / n
    |d dx| <= rs (u |gy| + d_m1 + |xh| d_m2 + |m2| d_xh + d_m2 d_xh + 3u (|gy| + |m1| + |xh m2|)) + u |dx0|  (+ u |dx| with dx_add)
    d_dgamma_c = (R + 3) u sum_r |dy xh| + sum_r |dy| d_xh,   d_dbeta_c = (R + 2) u sum_r |dy|
Softmax forward (z = x - m over the live columns):
    r_e = u |z| + X_RED u |z| + K_EXP u,   r = r_e + sum_j p_j r_e,j + (n_live + 5) u,   |d p| <= p r (1 + r) + 2^-126
    The first u |z| is the rounding of x - m.  The second (X_RED = 1) is inside the device expf as this library is built: its argument
    reduction takes PH = fl(z log2 e), the product's rounding error PL = fma(z, log2 e, -PH) and A = (PH - E) + PL with E = rint(PH); under
    -ffp-contract=fast the compiler fuses PH - E into fma(z, log2 e, -E), which already holds the exact difference, so PL (|PL| <= u |PH|)
    is counted twice and exp2(A) is off by PL ln 2 <= u |z| relative.  Seen on the MI355X at scores of scale 30 (z = -66: 1.09 of the
    bound without the term) and read from the ISA of softmax_fwd_kernel; a float64 model of the fused sequence gives exactly 1.000 u |z|.
Softmax backward (the stored p is an exact input):
    d_dot = (C + 2) u sum|g p|,   |d dx| <= |p| (d_dot + u (|g| + |dot|)) + u |dx| + 2^-126
    With dropout g = dy * keep_scale is itself one f32 product (softmax_bwd_kernel: ``g * keep_scale``), which adds u |g| inside the bracket;
    keep_scale enters the reference as the f32 value 1 / (1 - p) the kernel computes."""
import math

import torch

F32, BF16 = torch.float32, torch.bfloat16
U = 2.0 ** -24 * (1 + 2.0 ** -20)  # u, with room for the second-order terms ((1 + u)^k - 1 = k u + O(u^2))
TINY = 2.0 ** -126                 # results below the smallest normal f32 may be flushed to zero
K_RSQRT = 2                        # ulps of the device rsqrtf
K_EXP = 2                          # ulps of the device expf
X_RED = 1                          # u |z| of expf's argument reduction under -ffp-contract=fast (see above)


# ---------------------------------------------------------------------------------------------------------------------------------
# comparison helpers (shared with test_small_ops_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def half_ulp_bf16(mag):
    _, e = torch.frexp(mag)
    return torch.where(mag > 0, torch.ldexp(torch.ones_like(mag), e - 9), torch.zeros_like(mag))


def tol(ref, f32_err, dt):
    """f32 error bound -> bound on the stored result (plus the rounding to bf16 where the result is bf16)."""
    f32_err = torch.zeros_like(ref) + f32_err
    return f32_err + half_ulp_bf16(ref.abs() + f32_err) if dt == BF16 else f32_err


def check(got, ref, tol, what):
    """Element-wise |got - ref| <= tol (a NaN in ``got`` is outside; equal infinities are not).  Returns the largest err / tol."""
    assert tuple(got.shape) == tuple(ref.shape), "%s: shape %s vs %s" % (what, tuple(got.shape), tuple(ref.shape))
    g = got.double()
    err = (g - ref).abs()
    bad = ~((err <= tol) | (g == ref))  # a NaN in ``got`` is bad; equal infinities are not
    if bad.any():
        i = int(torch.where(bad, torch.nan_to_num(err, nan=float("inf")), torch.full_like(err, -1.0)).reshape(-1).argmax())
        raise AssertionError("%s: %d of %d elements outside the bound; flat index %d: got %r, want %r, bound %.3e" % (
            what, int(bad.sum()), bad.numel(), i, g.reshape(-1)[i].item(), ref.reshape(-1)[i].item(), (torch.zeros_like(ref) + tol).reshape(-1)[i].item()))
    t = torch.zeros_like(ref) + tol
    live = (err > 0) & (g != ref)
    return float(torch.where(live, err / t.clamp_min(1e-300), torch.zeros_like(err)).max()) if err.numel() else 0.0


class Stats(dict):
    """what -> [elements compared, largest err / bound]."""

    def add(self, what, n, ratio):
        cur = self.setdefault(what, [0, 0.0])
        cur[0] += int(n)
        cur[1] = max(cur[1], float(ratio))

    def check(self, got, ref, tol, what, label):
        self.add(what, ref.numel(), check(got, ref, tol, "%s %s" % (label, what)))

    def worst(self):
        return max([v[1] for v in self.values()] or [0.0])

    def elements(self):
        return sum(v[0] for v in self.values())


def same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    view = torch.int16 if got.dtype == BF16 else torch.int32
    a, b = got.contiguous().view(view), want.contiguous().view(view)
    assert torch.equal(a, b), "%s: %d elements differ in bits" % (what, int((a != b).sum()))


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm: inputs
# ---------------------------------------------------------------------------------------------------------------------------------
LN_EPS = 1e-5
LN_CLASSES = ("normal", "shift", "const", "gamma0")


def spike_columns(cols, dt, wave_cols=None):
    """Columns at which a dropped, duplicated or mis-owned element would sit: the ends of the first vector, of the first 64-lane chunk and
    of the row, and the first column of every wave's slice of a row-split kernel."""
    e = 4 if dt == F32 else 8
    want = [0, e - 1, 64 * e - 1, 64 * e, cols - e, cols - 1]
    if wave_cols:
        want += list(range(0, cols, wave_cols))
    return sorted({c for c in want if 0 <= c < cols})


def ln_inputs(rows, cols, dt, cls="normal", seed=0, x2=False, add=False, spike=None, dev="cpu"):
    """x, x2, dy, dx_add in ``dt`` (the rounded values ARE the inputs), gamma / beta in f32, eps.  ``spike``: a column that carries
    sqrt(cols) times the scale of the rest, in x and in dy."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * rows + cols)
    x = torch.randn(rows, cols, generator=g)
    dy = torch.randn(rows, cols, generator=g)
    xb = torch.randn(rows, cols, generator=g) * 0.5 if x2 else None
    extra = torch.randn(rows, cols, generator=g) if add else None
    gamma = 1.0 + 0.5 * torch.randn(cols, generator=g)
    beta = 0.5 * torch.randn(cols, generator=g)
    if cls == "shift":
        x = x + (100.0 if dt == F32 else 16.0)
    elif cls == "const":
        x[rows // 2] = 0.75
        if xb is not None:
            xb[rows // 2] = 0.25
    elif cls == "gamma0":
        gamma[::3] = 0.0
        gamma[1::3] = -gamma[1::3].abs()
    elif cls != "normal":
        raise ValueError(cls)
    if spike is not None:
        sign = 1.0 - 2.0 * (torch.arange(rows) % 2).float()
        x[:, spike] = math.sqrt(cols) * sign * (1.0 + 0.25 * torch.rand(rows, generator=g))
        dy[:, spike] = -math.sqrt(cols) * (1.0 + 0.25 * torch.rand(rows, generator=g))
    put = lambda t: None if t is None else t.to(dt).to(dev)
    return dict(rows=rows, cols=cols, dt=dt, x=put(x), x2=put(xb), dy=put(dy), dx_add=put(extra), gamma=gamma.to(dev), beta=beta.to(dev),
                eps=LN_EPS)


def ln_stats_f32(case):
    """The f32 mean / rstd a correct forward hands to the backward: float64 statistics of the rounded inputs, rounded to f32."""
    v = case["x"].double() + (case["x2"].double() if case["x2"] is not None else 0.0)
    mu = v.mean(-1)
    var = ((v - mu[:, None]) ** 2).mean(-1)
    eps = float(torch.tensor(case["eps"], dtype=F32))
    return mu.float(), ((var + eps) ** -0.5).float()


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm: references and checks
# ---------------------------------------------------------------------------------------------------------------------------------
def ln_fwd_ref(case):
    """-> dict(y, mean, rstd, tol_y (f32 part), tol_mean, tol_rstd), all float64."""
    x2 = case["x2"]
    h = 0.0 if x2 is None else 1.0
    v = case["x"].double() + (x2.double() if x2 is not None else 0.0)
    n = v.shape[-1]
    gamma, beta = case["gamma"].double(), case["beta"].double()
    eps = float(torch.tensor(case["eps"], dtype=F32))  # the kernel takes eps as a float
    mu = v.mean(-1, keepdim=True)
    d = v - mu
    s2 = (d * d).mean(-1, keepdim=True) + eps
    rs = s2 ** -0.5
    xh = d * rs
    y = xh * gamma + beta
    d_mu = (n + 2 + h) * U * v.abs().sum(-1, keepdim=True) / n
    d_d = d_mu + U * d.abs() + h * U * v.abs()
    r_var = (n + 8) * U + d_mu ** 2 / s2 + h * 2 * U * (d.abs() * v.abs()).sum(-1, keepdim=True) / (n * s2)
    r_rs = r_var / 2 + (K_RSQRT + 1) * U
    t_y = gamma.abs() * (rs * d_d * (1 + r_rs) + xh.abs() * (r_rs + 3 * U)) + U * y.abs() + U * beta.abs()
    return dict(y=y, mean=mu[:, 0], rstd=rs[:, 0], tol_y=t_y, tol_mean=(d_mu + U * mu.abs())[:, 0], tol_rstd=(r_rs * rs)[:, 0])


def ln_fwd_check(case, y, mean, rstd, stats, label):
    ref = ln_fwd_ref(case)
    stats.check(y, ref["y"], tol(ref["y"], ref["tol_y"], case["dt"]), "y", label)
    stats.check(mean, ref["mean"], ref["tol_mean"], "mean", label)
    stats.check(rstd, ref["rstd"], ref["tol_rstd"], "rstd", label)


def ln_bwd_ref(case, mean, rstd):
    """-> dict(dx, dgamma, dbeta, tol_dx (f32 part), tol_dgamma, tol_dbeta), float64; ``mean`` / ``rstd`` are the kernel's f32 inputs."""
    x2, extra = case["x2"], case["dx_add"]
    h = 0.0 if x2 is None else 1.0
    v = case["x"].double() + (x2.double() if x2 is not None else 0.0)
    R, n = v.shape
    gamma, dy = case["gamma"].double(), case["dy"].double()
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    xh = (v - mu) * rs
    gy = dy * gamma
    m1 = gy.mean(-1, keepdim=True)
    m2 = (gy * xh).mean(-1, keepdim=True)
    dx0 = rs * (gy - m1 - xh * m2)
    dx = dx0 + (extra.double() if extra is not None else 0.0)
    d_xh = U * xh.abs() + rs * (1 + U) * (U * (v - mu).abs() + h * U * v.abs())
    d_m1 = (n + 3) * U * gy.abs().sum(-1, keepdim=True) / n
    d_m2 = ((n + 4) * U * (gy * xh).abs().sum(-1, keepdim=True) + (gy.abs() * d_xh).sum(-1, keepdim=True)) / n
    t_dx = rs * (U * gy.abs() + d_m1 + xh.abs() * d_m2 + m2.abs() * d_xh + d_m2 * d_xh
                 + 3 * U * (gy.abs() + m1.abs() + (xh * m2).abs())) + U * dx0.abs()
    if extra is not None:
        t_dx = t_dx + U * dx.abs()
    t_dg = (R + 3) * U * (dy * xh).abs().sum(0) + (dy.abs() * d_xh).sum(0)
    t_db = (R + 2) * U * dy.abs().sum(0)
    return dict(dx=dx, dgamma=(dy * xh).sum(0), dbeta=dy.sum(0), tol_dx=t_dx, tol_dgamma=t_dg, tol_dbeta=t_db)


def ln_bwd_check(case, mean, rstd, dx, dgamma, dbeta, stats, label):
    ref = ln_bwd_ref(case, mean, rstd)
    stats.check(dx, ref["dx"], tol(ref["dx"], ref["tol_dx"], case["dt"]), "dx", label)
    stats.check(dgamma, ref["dgamma"], ref["tol_dgamma"], "dgamma", label)
    stats.check(dbeta, ref["dbeta"], ref["tol_dbeta"], "dbeta", label)
    return ref


def dropped_check(dx_stored, dx_dropped, p, keep, label):
    """dx_dropped is, element by element, 0 or round(dx_stored / (1 - p)) with the kernel's f32 scale 1 / (1 - p); its zero set is
    ``keep``'s complement (``keep``: case_dropout of a tensor of ones on the same (seed, offset), non-zero where kept)."""
    one = torch.tensor(1.0, dtype=F32)
    scale = (one / (one - torch.tensor(p, dtype=F32))).item()
    want = (dx_stored.float() * scale).to(dx_stored.dtype)
    want = torch.where(keep, want, torch.zeros_like(want))
    same_bits(dx_dropped, want, "%s dx_dropped" % label)
    return int(keep.sum())


def concat5_check(case, mean, rstd, row_valid, de, da1, da2, dgamma, dbeta, stats, label):
    """case_layernorm_bwd_concat5 on G = [E | A1 | A2 | E o A1 | E o A2] (bf16, H = cols / 5): dG from the LayerNorm backward, rounded
    to bf16 as the kernel and the two-kernel path do, then dE = dG0 + dG3 o A1 + dG4 o A2, dA1 = dG1 + dG3 o E, dA2 = dG2 + dG4 o E;
    padded rows are exact zeros; d_gamma / d_beta include the padded rows."""
    ref = ln_bwd_ref(case, mean, rstd)
    H = case["cols"] // 5
    x = case["x"].double()
    E, A1, A2 = (x[:, i * H:(i + 1) * H] for i in range(3))
    dG = [ref["dx"][:, i * H:(i + 1) * H] for i in range(5)]
    tG = [tol(ref["dx"], ref["tol_dx"], BF16)[:, i * H:(i + 1) * H] for i in range(5)]
    ok = row_valid.bool()[:, None]

    def piece(a, b, fb, c, fc):
        want = dG[a] + dG[b] * fb + dG[c] * fc
        mag = (dG[a].abs() + tG[a]) + (dG[b].abs() + tG[b]) * fb.abs() + (dG[c].abs() + tG[c]) * fc.abs()
        err = tG[a] + fb.abs() * tG[b] + fc.abs() * tG[c] + 2 * U * mag
        want, err = torch.where(ok, want, torch.zeros_like(want)), torch.where(ok, err, torch.zeros_like(err))
        return want, torch.where(ok, tol(want, err, BF16), torch.zeros_like(err))

    zero = torch.zeros_like(E)
    for name, got, (want, t) in (("de", de, piece(0, 3, A1, 4, A2)), ("da1", da1, piece(1, 3, E, 4, zero)),
                                 ("da2", da2, piece(2, 4, E, 3, zero))):
        stats.check(got, want, t, name, label)
    stats.check(dgamma, ref["dgamma"], ref["tol_dgamma"], "dgamma", label)
    stats.check(dbeta, ref["dbeta"], ref["tol_dbeta"], "dbeta", label)


# ---------------------------------------------------------------------------------------------------------------------------------
# softmax
# ---------------------------------------------------------------------------------------------------------------------------------
def softmax_inputs(outer, inner, R, C, in_dt, out_dt, seed=0, scale=1.0, cv=None, rv=False, causal=False, dev="cpu"):
    """Scores x [outer, inner, R, C] in ``in_dt``, an upstream gradient in ``out_dt``, col_valid [outer, C] / row_valid [outer, R] uint8.
    ``cv``: None, "half" (one half of the keys masked, the other half per outer) or "one" (a single masked column per outer)."""
    g = torch.Generator().manual_seed(977 * seed + 31 * C + R)
    x = torch.randn(outer, inner, R, C, generator=g) * scale
    dy = torch.randn(outer, inner, R, C, generator=g)
    col_valid = row_valid = None
    if cv is not None:
        col_valid = torch.ones(outer, C, dtype=torch.uint8)
        for o in range(outer):
            if cv == "half":
                lo = 0 if o % 2 else C // 2
                col_valid[o, lo:lo + max(C // 2, 1)] = 0
            elif cv == "one":
                col_valid[o, (3 * o + 1) % C] = 0
            else:
                raise ValueError(cv)
    if rv:
        row_valid = (torch.rand(outer, R, generator=g) < 0.7).to(torch.uint8)
        row_valid[0, 0] = 1
        row_valid[-1, -1] = 0
    put = lambda t: None if t is None else t.to(dev)
    return dict(outer=outer, inner=inner, R=R, C=C, in_dt=in_dt, out_dt=out_dt, causal=causal, x=x.to(in_dt).to(dev), dy=dy.to(out_dt).to(dev),
                col_valid=put(col_valid), row_valid=put(row_valid))


def softmax_live(case):
    """A column is live iff it passes row_valid, col_valid and causal and its score is finite or +inf."""
    x = case["x"]
    R, C = case["R"], case["C"]
    live = x.double() > -math.inf
    if case["col_valid"] is not None:
        live = live & case["col_valid"].bool()[:, None, None, :]
    if case["row_valid"] is not None:
        live = live & case["row_valid"].bool()[:, None, :, None]
    if case["causal"]:
        r = torch.arange(R, device=x.device)[:, None]
        c = torch.arange(C, device=x.device)[None, :]
        live = live & (c <= r)
    return live


def softmax_fwd_ref(case):
    """-> (p float64, f32 bound, live); a row without a live column is all zeros with bound 0."""
    live = softmax_live(case)
    x = case["x"].double()
    neg = torch.full_like(x, -math.inf)
    m = torch.where(live, x, neg).amax(-1, keepdim=True)
    any_live = live.any(-1, keepdim=True)
    z = torch.where(live, x - torch.where(any_live, m, torch.zeros_like(m)), torch.zeros_like(x))
    e = torch.where(live, torch.exp(z), torch.zeros_like(x))
    s = e.sum(-1, keepdim=True)
    p = e / torch.where(any_live, s, torch.ones_like(s))
    r_e = torch.where(live, (1 + X_RED) * U * z.abs() + K_EXP * U, torch.zeros_like(x))
    r = r_e + (p * r_e).sum(-1, keepdim=True) + (live.sum(-1, keepdim=True) + 5) * U
    bound = torch.where(live, p * r * (1 + r) + TINY, torch.zeros_like(x))
    return p, bound, live


def softmax_fwd_check(case, p_out, stats, label):
    p, bound, live = softmax_fwd_ref(case)
    stats.check(p_out, p, tol(p, bound, case["out_dt"]), "p", label)
    dead = ~live
    assert bool((p_out[dead] == 0).all()), "%s: a masked element is not exactly 0" % label
    return p, bound, live


def keep_scale_f32(p):
    one = torch.tensor(1.0, dtype=F32)
    return (one / (one - torch.tensor(p, dtype=F32))).item() if p > 0 else 1.0


def softmax_dropout_check(case, y_out, drop_p, stats, label, share=True):
    """y is 0 or within the bound of p_ref / (1 - p), and (``share``) at least 60 % of the unmasked elements were kept and so compared.
    Returns the keep set read from y (non-zero elements)."""
    p, bound, live = softmax_fwd_ref(case)
    scale = keep_scale_f32(drop_p)
    want = p * scale
    t = tol(want, bound * scale * (1 + 2 * U) + 2 * U * want, case["out_dt"])  # the f32 quotient 1 / (1 - p), then the product
    kept = y_out != 0
    assert not bool((kept & ~live).any()), "%s: dropout output outside the mask" % label
    g = y_out.double()
    bad = kept & ~((g - want).abs() <= t)
    assert not bool(bad.any()), "%s: %d kept elements outside the bound of p / (1 - p)" % (label, int(bad.sum()))
    ratio = torch.where(kept, (g - want).abs() / t.clamp_min(1e-300), torch.zeros_like(t))
    stats.add("y", int(kept.sum()), float(ratio.max()))
    unmasked = live & (p > 0)
    if not share:
        return kept
    share = float((kept & unmasked).sum()) / max(int(unmasked.sum()), 1)
    assert share >= 0.6, "%s: only %.2f of the unmasked elements were compared" % (label, share)
    assert share <= 0.8, "%s: %.2f of the unmasked elements kept at p = %.1f" % (label, share, drop_p)
    return kept


def softmax_bwd_ref(dy, p_stored, keep=None, drop_p=0.0):
    """From the stored p as an exact input; g is first masked and scaled by the keep set where there is one."""
    g, p = dy.double(), p_stored.double()
    C = p.shape[-1]
    h = 0.0
    if keep is not None:
        g = torch.where(keep, g * keep_scale_f32(drop_p), torch.zeros_like(g))
        h = 1.0
    dot = (g * p).sum(-1, keepdim=True)
    dx = p * (g - dot)
    d_dot = (C + 2) * U * (g * p).abs().sum(-1, keepdim=True)
    bound = p.abs() * (d_dot + U * ((1 + h) * g.abs() + dot.abs())) + U * dx.abs() + TINY
    return dx, torch.where(p == 0, torch.zeros_like(bound), bound)


def softmax_bwd_check(case, dy, p_stored, dx, stats, label, keep=None, drop_p=0.0):
    want, bound = softmax_bwd_ref(dy, p_stored, keep, drop_p)
    stats.check(dx, want, tol(want, bound, case["in_dt"]), "dx", label)
    assert bool((dx[p_stored == 0] == 0).all()), "%s: gradient where p is 0" % label
