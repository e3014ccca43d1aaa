"""Float64 references of the fused BatchNorm / GroupNorm (+ residual) (+ ReLU) kernels (csrc/bn_relu.hip, csrc/gn_relu.hip),
the elementwise error bounds that follow from the kernels' operation sequence, and the generator of their test inputs.
Plain numpy on closed formulas, no autograd, TEST INFRASTRUCTURE ONLY: nothing here touches ``gga_amd``. The inputs are the
float32 operands, converted exactly to double. tests/test_norm_ref.py pins this file to float64 autograd of torch before a
kernel is involved.

Error bounds (``*_bounds`` entries of the returned dicts): first-order propagation of ``u = 2**-24``
-----------------------------------------------------------------------------------------------------
Statistics. A thread of the reduce kernels adds ``x`` and ``x * x`` in float32 over a run of at most ``L`` elements of one
channel (``BN_RUN`` / ``GN_RUN`` below) and adds each finished run into float64; everything up to the casts of mean and
invstd is float64 from there (its error, ~n * 2**-53, is carried as ``F64``). Recursive summation of a run commits one
rounding per addition, each at most ``u`` times a partial sum, and a partial sum is at most the sum of the magnitudes
added so far. The element at position p of a run of length Lr therefore enters the bound with the number of additions it
takes part in, w = Lr - max(p, 1) <= L - 1 (the first addition, to zero, is exact):

    |S0' - S0| <= u sum w |x|                           |S1' - S1| <= u sum (w + 1) x^2   (one more rounding: the product)
    e_mu  = u mean(w |x|)
    e_var = u mean((w + 1) x^2) + 2 |mu| e_mu           (var' = S1'/n - mu'^2; the clamp at 0 only moves var' towards var)

With w <= L - 1, mean|x| <= sqrt(mean x^2) and |mu| <= sqrt(mean x^2) this is e_var <= (3 L - 2) u (var + mu^2) < 3 (L + 2)
u (var + mu^2): the bound grows with r^2 for r = |mu| / std, the price of the sum / sum-of-squares scheme. The helper
evaluates the first form with the data and with w from the kernels' own index arithmetic (``bn_run_weights``,
``gn_run_weights``): which element a thread reads at which step is fixed by the launch geometry, and a thread of a small
launch adds two elements (BatchNorm) or one row (GroupNorm), not a full run. Sums of g and g * x_hat in backward use the
same w; statistics that arrive as float64 partials (``run=1``) have w = 0.

    mean (f32)    e_mean = e_mu + u |mu|
    invstd (f32)  e_inv  = inv (e_var / (2 (var + eps)) + u)                 evaluation mode: 4 u inv (add, sqrtf, divide in f32)
    scale         e_sc   = |gamma| e_inv + u |sc|                              sc = gamma * inv
    shift         sh = beta - mean * sc, rounded: u (|mean sc| + |sh|)
    y             (x - mean') sc' + beta against (x - mu) sc + beta:
                  e_y = |x - mu| e_sc + |sc| e_mean + u (|mu sc| + |sh|) + u (|x sc| + |x sc + sh| + |pre|)
    running       e_rm = m e_mean + 3 u (|(1 - m) rm| + |m mu|),  e_rv likewise with e_unb = e_var n / (n - 1) + u unb
    x_hat (bwd)   e_xh = inv e_mean + |x_hat| (e_inv / inv + 2 u)
    sum g         e_sg = u sum w |g|
    sum g x_hat   e_sq = sum|g| e_xh + u sum (w + 1) |g x_hat|
    d_beta, d_gamma: those plus the cast, u |value|
    BatchNorm dx  k = gamma inv, mg = sum g / n, mgx = sum g x_hat / n, inner = g - mg - x_hat mgx
                  e_dx = |k| (e_mg + |x_hat| e_mgx + |mgx| e_xh + u (|g - mg| + |x_hat mgx| + |inner|)) + |inner| e_k + u |dx|
    GroupNorm dx  A = sum_c gamma_c sum g (f64), c1 = inv A / m, c2 likewise from sum g x_hat, dx = k g - c1 - x_hat c2
                  e_dx = |g| e_k + e_c1 + |x_hat| e_c2 + |c2| e_xh + u (|k g| + |k g - c1| + |x_hat c2| + |dx|)

Every returned bound is ``SAFETY`` times its first-order value; the factor covers the second-order terms dropped above.
A ReLU decision is not covered by any bound: the generator below keeps every pre-activation away from zero instead, so
mask, dx and d_residual are compared at every element.
"""
import numpy as np

U = 2.0 ** -24
F64 = 2.0 ** -53
BN_RUN = 16          # 8 * BN_U: `if (++run == 8)` in bn_reduce_kernel, csrc/bn_relu.hip
GN_RUN = 32          # 8 * GN_U: `if (++run == 8)` in gn_reduce_kernel, csrc/gn_relu.hip
SAFETY = 2.0
MARGIN = 100.0       # ReLU decisions: no pre-activation within MARGIN * (bound on y) of zero


def f64(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.astype(np.float64)


def _f32(v):
    return float(np.float32(v))


BN_MAX_BLOCKS, BN_U, GN_CHUNKS = 2048, 2, 64      # csrc/bn_relu.hip, csrc/gn_relu.hip


def _run_weights(k, kmax, run):
    """Additions that the k-th element of a thread takes part in, for a thread of at most kmax elements in runs of `run`."""
    p, j = k % run, k // run
    return np.maximum(np.minimum(run, kmax - j * run) - np.maximum(p, 1), 0).astype(np.float64)


def bn_run_weights(n, C, run=BN_RUN):
    """[n, C]: thread e0 of bn_reduce_kernel reads float4 e0 + k * stride, stride = 256 * bn_grid(n4), k = 0, 1, ..."""
    if run == 1:
        return np.zeros((1, C))
    c4 = C // 4
    n4 = n * c4
    grid = min(BN_MAX_BLOCKS, max(1, -(-n4 // (256 * BN_U))))
    stride = grid * 256
    e = np.arange(n, dtype=np.int64)[:, None] * c4 + np.arange(c4, dtype=np.int64)[None, :]
    return np.repeat(_run_weights(e // stride, -(-n4 // stride), run), 4, axis=1)


def gn_run_weights(R, C, run=GN_RUN):
    """[R, 1]: a workgroup of gn_reduce_kernel takes rows R * chunk / 64 .. R * (chunk + 1) / 64, 256 / (C / 4) rows at a time."""
    rstep = 256 // (C // 4)
    w = np.zeros(R)
    for chunk in range(GN_CHUNKS):
        rb, re = R * chunk // GN_CHUNKS, R * (chunk + 1) // GN_CHUNKS
        if re > rb:
            w[rb:re] = _run_weights(np.arange(re - rb) // rstep, -(-(re - rb) // rstep), run)
    return w[:, None]


# --------------------------------------------------------------------------------------------------- BatchNorm
def bn_forward(x, gamma, beta, running_mean, running_var, eps, momentum, training, relu, residual=None, rows=None,
               run=BN_RUN):
    """BatchNorm over x [n, C]. ``rows``: the rows (index array) for which the elementwise outputs are returned (all when
    None); the statistics always cover every row. Returns a dict of float64 values and, under ``bounds``, their bounds."""
    x, gamma, beta = f64(x), f64(gamma), f64(beta)
    rm, rv = f64(running_mean), f64(running_var)
    n, C = x.shape
    eps, m = _f32(eps), _f32(momentum)
    o, b = {}, {}
    if training:
        mu = x.mean(0)
        var = ((x - mu) ** 2).mean(0)
        w = bn_run_weights(n, C, run)
        e_mu = U * (w * np.abs(x)).mean(0) + n * F64 * np.abs(x).mean(0)
        e_var = U * ((w + 1.0) * x * x).mean(0) + n * F64 * (x * x).mean(0) + 2.0 * np.abs(mu) * e_mu
        inv = 1.0 / np.sqrt(var + eps)
        e_mean = e_mu + U * np.abs(mu)
        e_inv = inv * (0.5 * e_var / (var + eps) + U)
        unb = var * n / (n - 1) if n > 1 else var            # the kernel's definition for one row
        e_unb = (e_var * n / (n - 1) if n > 1 else e_var) + U * unb
        o['running_mean'] = (1.0 - m) * rm + m * mu
        o['running_var'] = (1.0 - m) * rv + m * unb
        b['running_mean'] = m * e_mean + 3 * U * (np.abs((1.0 - m) * rm) + np.abs(m * mu))
        b['running_var'] = m * e_unb + 3 * U * (np.abs((1.0 - m) * rv) + np.abs(m * unb))
    else:
        mu, var = rm, rv
        inv = 1.0 / np.sqrt(var + eps)
        e_mean, e_var, e_inv = np.zeros(C), np.zeros(C), 4 * U * inv
        o['running_mean'], o['running_var'] = rm, rv
        b['running_mean'] = b['running_var'] = np.zeros(C)
    xs = x if rows is None else x[rows]
    sc = gamma * inv
    sh = beta - mu * sc
    e_sc = np.abs(gamma) * e_inv + U * np.abs(sc)
    pre = (xs - mu) * sc + beta
    if residual is not None:
        pre = pre + (f64(residual) if rows is None else f64(residual)[rows])
    e_y = (np.abs(xs - mu) * e_sc + np.abs(sc) * e_mean + U * (np.abs(mu * sc) + np.abs(sh))
           + U * (np.abs(xs * sc) + np.abs(xs * sc + sh) + np.abs(pre)))
    o.update(mean=mu, var=var, invstd=inv, scale=sc, pre=pre, mask=(pre > 0.0) if relu else np.ones(pre.shape, bool))
    o['y'] = np.maximum(pre, 0.0) if relu else pre
    b.update(mean=e_mean, var=e_var, invstd=e_inv, y=e_y)
    o['bounds'] = {k: SAFETY * v for k, v in b.items()}
    o['_e'] = dict(mean=e_mean, inv=e_inv)
    o['n'], o['rows'], o['training'], o['run'] = n, rows, bool(training), run
    return o


def bn_backward(x, dy, gamma, fwd, mask=None):
    """Backward of ``bn_forward`` (its result is ``fwd``); ``mask`` [n, C] when ``fwd`` holds only some rows. Sums over all
    rows, dx / d_residual on ``fwd['rows']``."""
    x, dy, gamma = f64(x), f64(dy), f64(gamma)
    n, rows, run = fwd['n'], fwd['rows'], fwd['run']
    mask = fwd['mask'] if mask is None else mask
    assert mask.shape == x.shape
    mu, inv, e_mean, e_inv = fwd['mean'], fwd['invstd'], fwd['_e']['mean'], fwd['_e']['inv']
    w = bn_run_weights(n, x.shape[1], run)
    g = dy * mask
    xh = (x - mu) * inv
    sg, sq = g.sum(0), (g * xh).sum(0)
    ag, aq = np.abs(g).sum(0), np.abs(g * xh).sum(0)
    rel_xh = e_inv / inv + 2 * U
    e_sg = U * (w * np.abs(g)).sum(0) + n * F64 * ag
    e_sq = inv * e_mean * ag + rel_xh * aq + U * ((w + 1.0) * np.abs(g * xh)).sum(0) + n * F64 * aq
    o = dict(d_beta=sg, d_gamma=sq)
    b = dict(d_beta=e_sg + U * np.abs(sg), d_gamma=e_sq + U * np.abs(sq))
    tr = 1.0 if fwd['training'] else 0.0
    mg, mgx = tr * sg / n, tr * sq / n
    e_mg, e_mgx = tr * (e_sg / n + U * np.abs(mg)), tr * (e_sq / n + U * np.abs(mgx))
    k = gamma * inv
    e_k = np.abs(gamma) * e_inv + U * np.abs(k)
    g_all, xh_all = g, xh
    if rows is not None:
        g, xh = g[rows], xh[rows]
    e_xh = inv * e_mean + np.abs(xh) * rel_xh
    inner = g - mg - xh * mgx
    dx = k * inner
    e_inner = e_mg + np.abs(xh) * e_mgx + np.abs(mgx) * e_xh + U * (np.abs(g - mg) + np.abs(xh * mgx) + np.abs(inner))
    b['dx'] = np.abs(k) * e_inner + np.abs(inner) * e_k + U * np.abs(dx)
    o.update(dx=dx, d_residual=g, g_all=g_all, xhat_all=xh_all)
    o['bounds'] = {k_: SAFETY * v for k_, v in b.items()}
    return o


def column_sums(x, run=BN_RUN):
    x = f64(x)
    n = x.shape[0]
    s = x.sum(0)
    w = bn_run_weights(n, x.shape[1], run)
    return s, SAFETY * (U * (w * np.abs(x)).sum(0) + n * F64 * np.abs(x).sum(0) + U * np.abs(s))


def partial_sums(a, b, n_partials):
    """[n_partials, 2, C] float64: column sums of a and b over the row groups i % n_partials (what a producer's tiles leave)."""
    n, C = a.shape
    out = np.zeros((n_partials, 2, C))
    for p in range(min(n_partials, n)):
        out[p, 0], out[p, 1] = a[p::n_partials].sum(0), b[p::n_partials].sum(0)
    return out


# --------------------------------------------------------------------------------------------------- GroupNorm
def gn_forward(x, gamma, beta, groups, eps, relu, run=GN_RUN):
    """GroupNorm over x [B, R, C] (the memory of a channels-last [B, C, H, W] tensor), statistics per (sample, group)."""
    x, gamma, beta = f64(x), f64(gamma), f64(beta)
    B, R, C = x.shape
    G, gs = groups, C // groups
    eps = _f32(eps)
    xg = x.reshape(B, R, G, gs)
    mu = xg.mean((1, 3))
    var = ((xg - mu[:, None, :, None]) ** 2).mean((1, 3))
    w = gn_run_weights(R, C, run)[None, :, :, None]                      # [1, R, 1, 1]: a thread adds rows of one channel
    mabs, msq = np.abs(xg).mean((1, 3)), (xg * xg).mean((1, 3))
    e_mu = U * (w * np.abs(xg)).mean((1, 3)) + R * gs * F64 * mabs
    e_var = U * ((w + 1.0) * xg * xg).mean((1, 3)) + R * gs * F64 * msq + 2.0 * np.abs(mu) * e_mu
    inv = 1.0 / np.sqrt(var + eps)
    e_mean = e_mu + U * np.abs(mu)
    e_inv = inv * (0.5 * e_var / (var + eps) + U)
    ch = lambda a: np.repeat(a, gs, axis=1)[:, None, :]               # [B, G] -> [B, 1, C]
    muc, invc = ch(mu), ch(inv)
    sc = gamma * invc
    sh = beta - muc * sc
    e_sc = np.abs(gamma) * ch(e_inv) + U * np.abs(sc)
    pre = (x - muc) * sc + beta
    e_y = (np.abs(x - muc) * e_sc + np.abs(sc) * ch(e_mean) + U * (np.abs(muc * sc) + np.abs(sh))
           + U * (np.abs(x * sc) + np.abs(x * sc + sh) + np.abs(pre)))
    o = dict(mean=mu, var=var, invstd=inv, scale=sc, pre=pre, mask=(pre > 0.0) if relu else np.ones(pre.shape, bool))
    o['y'] = np.maximum(pre, 0.0) if relu else pre
    o['bounds'] = {k: SAFETY * v for k, v in dict(mean=e_mean, var=e_var, invstd=e_inv, y=e_y).items()}
    o['_e'] = dict(mean=e_mean, inv=e_inv)
    o['groups'], o['run'] = G, run
    return o


def gn_backward(x, dy, gamma, fwd):
    x, dy, gamma = f64(x), f64(dy), f64(gamma)
    B, R, C = x.shape
    G, run = fwd['groups'], fwd['run']
    gs = C // G
    w = gn_run_weights(R, C, run)[None]                                  # [1, R, 1]
    m = R * gs
    ch = lambda a: np.repeat(a, gs, axis=1)[:, None, :]
    grp = lambda a: a.reshape(B, G, gs).sum(2)                          # [B, C] -> [B, G]
    mu, inv, e_mean, e_inv = ch(fwd['mean']), ch(fwd['invstd']), ch(fwd['_e']['mean']), ch(fwd['_e']['inv'])
    g = dy * fwd['mask']
    xh = (x - mu) * inv
    s, q = g.sum(1), (g * xh).sum(1)                                    # [B, C]
    ag, aq = np.abs(g).sum(1), np.abs(g * xh).sum(1)
    rel_xh = e_inv / inv + 2 * U
    e_s = U * (w * np.abs(g)).sum(1) + R * F64 * ag
    e_q = (inv * e_mean)[:, 0] * ag + rel_xh[:, 0] * aq + U * ((w + 1.0) * np.abs(g * xh)).sum(1) + R * F64 * aq
    o = dict(d_beta=s.sum(0), d_gamma=q.sum(0))
    b = dict(d_beta=e_s.sum(0) + U * np.abs(o['d_beta']), d_gamma=e_q.sum(0) + U * np.abs(o['d_gamma']))
    A, Bq = grp(gamma * s), grp(gamma * q)
    e_A, e_B = grp(np.abs(gamma) * e_s), grp(np.abs(gamma) * e_q)
    ginv, ge_inv = fwd['invstd'], fwd['_e']['inv']
    c1, c2 = ch(ginv * A / m), ch(ginv * Bq / m)
    e_c1 = ch((ginv * e_A + ge_inv * np.abs(A)) / m) + U * np.abs(c1)
    e_c2 = ch((ginv * e_B + ge_inv * np.abs(Bq)) / m) + U * np.abs(c2)
    k = gamma * inv
    e_k = np.abs(gamma) * e_inv + U * np.abs(k)
    e_xh = inv * e_mean + np.abs(xh) * rel_xh
    dx = k * g - c1 - xh * c2
    b['dx'] = (np.abs(g) * e_k + e_c1 + np.abs(xh) * e_c2 + np.abs(c2) * e_xh
               + U * (np.abs(k * g) + np.abs(k * g - c1) + np.abs(xh * c2) + np.abs(dx)))
    o['dx'] = dx
    o['bounds'] = {k_: SAFETY * v for k_, v in b.items()}
    return o


# --------------------------------------------------------------------------------------------------- inputs
def _frac(i, a):
    return (np.asarray(i, np.float64) * a) % 1.0


def unit_loc_scale(n):
    """Location and scale of statistic i of n (a BatchNorm channel, a GroupNorm (sample, group)): scales 2**-3 .. 2**3 in a
    cycle of 7, r = loc / scale distinct in [-0.5, 0.5] - no two units share a distribution, so an exchange of channels,
    quads, groups or samples moves the statistics by far more than any bound."""
    i = np.arange(n)
    scale = 2.0 ** (i % 7 - 3)
    return (_frac(i + 1, 0.6180339887498949) - 0.5) * scale, scale


def affine(C):
    """gamma of both signs and magnitude 0.5 .. 1.5, beta in -0.5 .. 0.5, distinct per channel."""
    c = np.arange(C)
    gamma = (0.5 + _frac(c + 1, 0.3819660112501051)) * np.where(c % 3 == 2, -1.0, 1.0)
    return gamma.astype(np.float32), (_frac(c + 1, 0.7548776662466927) - 0.5).astype(np.float32)


def _nudge(x, relu, evaluate, what):
    """Repeat until no pre-activation lies within MARGIN * bound of zero: such elements of x are pushed away from the ReLU
    boundary on the side they are on. Returns x; the condition is zero excluded elements."""
    if not relu:
        return x
    for _ in range(20):
        pre, e_y, sc = evaluate(x)
        near = np.abs(pre) < MARGIN * e_y
        if not near.any():
            return x
        sc = np.broadcast_to(sc, pre.shape)
        assert (sc[near] != 0).all(), f'{what}: a pre-activation near zero under a zero scale cannot be moved'
        step = 4.0 * MARGIN * e_y[near] / np.abs(sc[near]) * np.where(pre[near] >= 0, 1.0, -1.0) * np.sign(sc[near])
        x = x.copy()
        x[near] = (x[near].astype(np.float64) + step).astype(np.float32)
    raise AssertionError(f'{what}: {int(near.sum())} pre-activations still within the margin of zero')


def relu_margin_violations(pre, e_y):
    """Elements whose ReLU decision a rounding error could change (the generator's condition: 0)."""
    return int((np.abs(pre) < MARGIN * e_y).sum())


def make_bn_case(n, C, seed=0, relu=True, residual=False, training=True, eps=1e-3, momentum=0.01, r=None, r_channel=1):
    """Inputs of one BatchNorm case as float32 arrays. ``r``: |mean| / std of channel ``r_channel`` (conditioning cases)."""
    rng = np.random.default_rng(seed)
    loc, scale = unit_loc_scale(C)
    if r is not None:
        loc[r_channel] = r * scale[r_channel]
    gamma, beta = affine(C)
    x = (rng.standard_normal((n, C), np.float32) * scale.astype(np.float32) + loc.astype(np.float32)).astype(np.float32)
    res = (rng.standard_normal((n, C), np.float32) * 0.5).astype(np.float32) if residual else None
    rm = (loc + 0.1 * scale).astype(np.float32)
    rv = (1.3 * scale * scale).astype(np.float32)
    case = dict(gamma=gamma, beta=beta, running_mean=rm, running_var=rv, eps=eps, momentum=momentum, training=training,
                relu=relu, residual=res, n=n, C=C)

    def evaluate(xx):
        f = bn_forward(xx, gamma, beta, rm, rv, eps, momentum, training, relu, res)
        return f['pre'], f['bounds']['y'], f['scale']
    x = _nudge(x, relu, evaluate, f'bn {n}x{C}')
    c = np.arange(C)
    ds = 2.0 ** (c % 5 - 2)
    # a gradient whose per-channel sums and correlation with x_hat are far from zero: the mean(g) and mean(g x_hat) terms
    # of dx carry weight, and d_gamma / d_beta are not sums that cancel
    f = lambda a: np.asarray(a, np.float32)
    dy = f(ds) * (f(0.5 / scale) * (x - f(loc)) + f(np.where(c % 2 == 0, 0.5, -0.5)) + f(0.5) * rng.standard_normal((n, C), np.float32))
    case.update(x=x, dy=dy)
    return case


def bn_case_forward(case, rows=None, **kw):
    a = dict(case, **kw)
    return bn_forward(a['x'], a['gamma'], a['beta'], a['running_mean'], a['running_var'], a['eps'], a['momentum'],
                      a['training'], a['relu'], a['residual'], rows=rows, run=a.get('run', BN_RUN))


def make_gn_case(B, C, G, H, W, seed=0, relu=True, eps=1e-5, r=None, r_unit=1):
    """Inputs of one GroupNorm case: x, dy as float32 [B, H*W, C] (channels-last memory). ``r``: |mean| / std of (sample,
    group) number ``r_unit`` (conditioning cases)."""
    rng = np.random.default_rng(seed)
    R, gs = H * W, C // G
    loc, scale = unit_loc_scale(B * G)
    if r is not None:
        loc[r_unit] = r * scale[r_unit]
    locc = np.repeat(loc.reshape(B, G), gs, axis=1)[:, None, :]
    scc = np.repeat(scale.reshape(B, G), gs, axis=1)[:, None, :]
    gamma, beta = affine(C)
    x = (rng.standard_normal((B, R, C), np.float32) * scc.astype(np.float32) + locc.astype(np.float32)).astype(np.float32)

    def evaluate(xx):
        f = gn_forward(xx, gamma, beta, G, eps, relu)
        return f['pre'], f['bounds']['y'], f['scale']
    x = _nudge(x, relu, evaluate, f'gn {B}x{C}x{H}x{W}/{G}')
    c = np.arange(C)
    ds = 2.0 ** (c % 5 - 2)
    f = lambda a: np.asarray(a, np.float32)
    dy = f(ds) * (f(0.5 / scc) * (x - f(locc)) + f(np.where(c % 2 == 0, 0.5, -0.5)) + f(0.5) * rng.standard_normal((B, R, C), np.float32))
    return dict(x=x, dy=dy, gamma=gamma, beta=beta, groups=G, eps=eps, relu=relu, shape=(B, C, H, W))


# --------------------------------------------------------------------------------------------------- the listed cases
BN_SHAPES = [(1, 4), (2, 8), (3, 1024), (63, 16), (64, 16), (65, 16), (511, 4), (512, 4), (513, 4), (3 * 5 * 7, 8)]
BN_CAPPED = (2 * 132 * 125, 128)         # grid capped at BN_MAX_BLOCKS, second partial run
BN_FLUSH = (524293, 64)                  # just past the f32 -> f64 flush: 2048 x 256 x 16 float4 + 80
BN_MODES = [(True, False), (False, False), (True, True), (False, True)]          # (relu, residual)
GN_SHAPES = [(1, 4, 1, 1, 1), (2, 8, 2, 1, 3), (1, 32, 8, 7, 9), (2, 64, 16, 8, 8), (1, 64, 1, 5, 13), (1, 1024, 32, 3, 5)]
GN_FLUSH = (1, 256, 32, 96, 96)          # 144 rows per chunk over 4 row slots: 36 > 32 rows per thread
BN_COND, GN_COND = (65, 16), (2, 64, 16, 8, 8)
COND_BOUNDED, COND_RECORDED = (0.0, 1.0, 30.0), (1e3, 1e5)
