"""Paged-decode checker shared by the decode tests (a plain helper module, not a conftest).

reference(): the one fp64 statement of decode's semantics as include/mio_hip.h gives them, on the CPU: q [B,H,q_len,D]
over the paged cache [num_blocks, L, block_size, Hkv, D]; no causal mask among the q_len rows; with a window (left >= 0)
row qi sees the keys ctx - q_len + qi - left <= j < ctx; keys at positions >= max_blocks * block_size do not exist; an
fp8 cache stands for x8 * scale; a row with no visible key is o = 0, lse = -inf.  It gathers only the slots
0 .. min(ctx, max_blocks * block_size) - 1 of each sequence, the slots a kernel may read.

model(): the same operation as a plain fp32 online-softmax chain over 128-key blocks, rounded to the storage dtype at
the end; with p16 the weights are rounded to the dtype before the P.V product and summed as rounded (what the
matrix-core kernel does).  It shares no code with the kernels and is the yardstick the bars are taken from.

hostile_cache(): caches and block tables in which every slot no sequence owns at the tested layer (positions >= ctx in
owned blocks, unowned blocks, all of the other layers) is NaN (fp8: the e4m3fn NaN byte 0x7f), and every table entry past
a sequence's last needed block names one all-NaN block inside the cache: a kernel that lets such a slot into the result,
at whatever weight, returns NaN.

check(): every output finite; rows without a visible key exactly 0; per-row normwise error ||o - ref|| / ||ref|| in units
of the dtype's unit roundoff u (bf16 2^-8, fp16 2^-11) as three statistics: the worst row, the mean over live rows and
the worst mean over the rows of one sequence (the unit a wrong split, merge or block-table walk corrupts).  The bars are
the same statistics of model() on the same inputs times MARGINS, each floored at FLOOR u (a batch of one-key contexts
has model error 0; the floor is the rounding of the output itself plus slack).  Where MARGINS comes from: the fp32 chain
sits at 0.45-0.70 u worst and 0.38-0.57 u mean over contexts 33 / 300 / 5000 on randn, V = 1 + 0.05 randn and
dominating-key data; the attention-forward kernels of the same construction (MFMA, exp2, 16-bit P) measure up to 1.9 u
worst and 0.62 u mean on the MI355X (tests/_attn_check.py), about 3x and 1.25x such a model; the smallest defect that
tests/test_decode_check.py injects (one key of 4096 lost) is 5.9 u in bf16, 8x the model.  Margins are never per case.

STATS collects, per (q dtype, route, cache kind, windowed), the maxima over a process's check() calls of the kernel's
and the model's statistics and of their ratios to the bars.

Measured on the MI355X by one run of tests/test_gpu_decode_matrix.py (largest value per family over its cases, kernel /
model, in u; "ratio" is the largest statistic / bar over the three statistics and all cases, 1.0 = at the bar):

  q dtype  route  cache  window |  kernel: worst   mean    seq  |  model: worst   mean    seq  | ratio   n
  bfloat16 gqa    fp8    no     |          0.72  0.577   0.58  |         0.72  0.606   0.61  |  0.63   6
  bfloat16 gqa    fp8    yes    |          0.81  0.558   0.62  |         0.78  0.575   0.65  |  0.65   8
  bfloat16 gqa    kv16   no     |          0.70  0.559   0.56  |         0.72  0.566   0.58  |  0.66   7
  bfloat16 gqa    kv16   yes    |          0.70  0.505   0.59  |         0.72  0.546   0.61  |  0.66   9
  bfloat16 head   fp8    no     |          0.67  0.430   0.55  |         0.67  0.430   0.55  |  0.57   5
  bfloat16 head   fp8    yes    |          0.61  0.427   0.47  |         0.61  0.427   0.47  |  0.57   9
  bfloat16 head   kv16   no     |          0.73  0.413   0.52  |         0.73  0.413   0.52  |  0.55   6
  bfloat16 head   kv16   yes    |          0.76  0.424   0.48  |         0.76  0.424   0.48  |  0.57   8
  bfloat16 rows   fp8    no     |          0.58  0.434   0.48  |         0.58  0.434   0.48  |  0.58   5
  bfloat16 rows   fp8    yes    |          0.56  0.444   0.48  |         0.56  0.444   0.48  |  0.59   9
  bfloat16 rows   kv16   no     |          0.57  0.405   0.50  |         0.57  0.405   0.50  |  0.54   5
  bfloat16 rows   kv16   yes    |          0.63  0.431   0.47  |         0.63  0.431   0.47  |  0.57   8
  float16  gqa    fp8    no     |          0.61  0.499   0.53  |         0.68  0.535   0.56  |  0.64   6
  float16  gqa    fp8    yes    |          0.67  0.514   0.57  |         0.68  0.532   0.58  |  0.65   6
  float16  gqa    kv16   no     |          0.60  0.456   0.50  |         0.70  0.476   0.55  |  0.61   5
  float16  gqa    kv16   yes    |          0.73  0.554   0.56  |         0.86  0.603   0.62  |  0.64   6
  float16  head   fp8    no     |          0.70  0.454   0.53  |         0.70  0.454   0.53  |  0.60   5
  float16  head   fp8    yes    |          0.63  0.425   0.51  |         0.63  0.425   0.51  |  0.57   6
  float16  head   kv16   no     |          0.70  0.455   0.54  |         0.70  0.455   0.54  |  0.61   5
  float16  head   kv16   yes    |          0.55  0.424   0.48  |         0.55  0.424   0.48  |  0.57   6
  float16  rows   fp8    no     |          0.55  0.446   0.48  |         0.55  0.446   0.48  |  0.59   5
  float16  rows   fp8    yes    |          0.62  0.433   0.47  |         0.62  0.433   0.47  |  0.58   6
  float16  rows   kv16   no     |          0.55  0.428   0.50  |         0.55  0.428   0.50  |  0.57   6
  float16  rows   kv16   yes    |          0.55  0.396   0.45  |         0.55  0.396   0.45  |  0.53   6

  (154 tests in 8.8 s of wall time; tests/test_gpu_attention_matrix.py took 3.2 s in the same run.  Nearly all of the
  time here is the CPU: drawing the caches, the fp64 reference and the fp32 model.)
  The vector-ALU kernels (head, rows) keep fp32 throughout and land on the model's figures to the digits shown: what is
  left is the rounding of the output.  The matrix-core kernel sits at or slightly below its 16-bit-P model.  No family
  comes near a margin, so MARGINS stands at 3 / 1.5 / 2 with the floor of 0.75 u, none widened.  The bar that comes
  closest is the mean (1.5 x the model's mean, or the floor): the largest statistic-to-bar ratio measured is 0.66.

CASES is the case table of tests/test_gpu_decode_matrix.py with the route each case must take; tests/test_decode_check.py
confirms the routes on the CPU through the host-only route queries and checks the table's coverage.
"""
from __future__ import annotations

import math
import random

import torch

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
F8 = torch.float8_e4m3fn
F8_NAN = 0x7F
BLOCK = 128                      # keys per step of model()'s chain
MARGINS = {"worst": 3.0, "mean": 1.5, "seq": 2.0}   # kernel statistic <= margin x model statistic ...
FLOOR = 0.75                     # ... or this many u, whichever is larger

STATS: dict = {}


# ---- the reference --------------------------------------------------------------------------------------------------
def seq_len_eff(ctx, max_blocks, block_size):
    """Keys of a sequence that exist: those inside its block-table row."""
    return max(0, min(int(ctx), int(max_blocks) * int(block_size)))


def seq_kv(k_cache, v_cache, bt_row, n, block_size, layer, k_scale=1.0, v_scale=1.0, dtype=torch.float64):
    """K, V [n, Hkv, D] of the first n keys of a sequence (fp8: dequantised), in `dtype`."""
    pos = torch.arange(n)
    blk = bt_row[pos // block_size].long()
    slot = pos % block_size
    k, v = k_cache[blk, layer, slot], v_cache[blk, layer, slot]
    if k.dtype == F8:
        k, v = k.float(), v.float()   # exact
    return k.to(dtype) * k_scale, v.to(dtype) * v_scale


def seq_visible(ctx, n, q_len, left):
    """[q_len, n] bool: which of the keys 0 .. n-1 each query row of a sequence of length ctx sees."""
    vis = torch.ones(q_len, n, dtype=torch.bool)
    if left >= 0:
        lo = int(ctx) - q_len + torch.arange(q_len).view(q_len, 1) - left
        vis = torch.arange(n).view(1, n) >= lo
    return vis


def seq_attention(qb, k, v, scale, vis):
    """fp64 attention of one sequence: qb [H, q_len, D], k / v [n, Hkv, D], vis [q_len, n] -> (o [H,q_len,D], lse
    [H,q_len]); rows that see nothing are o = 0, lse = -inf."""
    H, q_len, D = qb.shape
    n, Hkv = k.shape[0], k.shape[1]
    if n == 0:
        return torch.zeros(H, q_len, D, dtype=torch.float64), torch.full((H, q_len), float("-inf"), dtype=torch.float64)
    kk = k.repeat_interleave(H // Hkv, dim=1)
    vv = v.repeat_interleave(H // Hkv, dim=1)
    s = torch.einsum("hqd,nhd->hqn", qb.double(), kk) * scale
    s = s.masked_fill(~vis.view(1, q_len, n), float("-inf"))
    m = s.amax(dim=-1)
    empty = torch.isinf(m) & (m < 0)
    p = torch.exp(s - torch.where(empty, torch.zeros_like(m), m)[..., None])
    p = torch.where(empty[..., None], torch.zeros_like(p), p)
    l = p.sum(-1)
    lse = torch.where(empty, m, m + torch.log(l))
    o = torch.einsum("hqn,nhd->hqd", p / torch.where(empty, torch.ones_like(l), l)[..., None], vv)
    return o, lse


def reference(q, k_cache, v_cache, block_tables, ctx, block_size, layer, *, left=-1, scale=None, k_scale=1.0,
              v_scale=1.0):
    """fp64 (o [B,H,q_len,D], lse [B,H,q_len]) of one paged decode launch, on the CPU."""
    B, H, q_len, D = q.shape
    sc = (1.0 / math.sqrt(D)) if scale is None else float(scale)
    o = torch.zeros(B, H, q_len, D, dtype=torch.float64)
    lse = torch.full((B, H, q_len), float("-inf"), dtype=torch.float64)
    for b in range(B):
        n = seq_len_eff(ctx[b], block_tables.shape[1], block_size)
        if n == 0:
            continue
        k, v = seq_kv(k_cache, v_cache, block_tables[b], n, block_size, layer, float(k_scale), float(v_scale))
        o[b], lse[b] = seq_attention(q[b], k, v, sc, seq_visible(ctx[b], n, q_len, left))
    return o, lse


# ---- the model ------------------------------------------------------------------------------------------------------
def model(q, k_cache, v_cache, block_tables, ctx, block_size, layer, *, dtype, p16, left=-1, scale=None, k_scale=1.0,
          v_scale=1.0):
    """The decode as an fp32 online-softmax chain over BLOCK-key steps, rounded to `dtype`: [B,H,q_len,D] in dtype."""
    B, H, q_len, D = q.shape
    f32 = torch.float32
    sc = torch.tensor((1.0 / math.sqrt(D)) if scale is None else float(scale), dtype=f32)
    ks, vs = torch.tensor(float(k_scale), dtype=f32), torch.tensor(float(v_scale), dtype=f32)
    out = torch.zeros(B, H, q_len, D, dtype=dtype)
    for b in range(B):
        n = seq_len_eff(ctx[b], block_tables.shape[1], block_size)
        if n == 0:
            continue
        k, v = seq_kv(k_cache, v_cache, block_tables[b], n, block_size, layer, ks, vs, dtype=f32)
        rep = H // k.shape[1]
        k = k.repeat_interleave(rep, dim=1).permute(1, 0, 2)   # [H, n, D]
        v = v.repeat_interleave(rep, dim=1).permute(1, 0, 2)
        vis = seq_visible(ctx[b], n, q_len, left)
        qb = q[b].to(f32)
        m = torch.full((H, q_len), float("-inf"), dtype=f32)
        l = torch.zeros(H, q_len, dtype=f32)
        acc = torch.zeros(H, q_len, D, dtype=f32)
        for a in range(0, n, BLOCK):
            e = min(a + BLOCK, n)
            s = torch.matmul(qb, k[:, a:e].transpose(1, 2)) * sc
            s = s.masked_fill(~vis[:, a:e].view(1, q_len, e - a), float("-inf"))
            m_new = torch.maximum(m, s.amax(dim=-1))
            m_ref = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
            alpha = torch.exp(m - m_ref)
            p = torch.exp(s - m_ref[..., None])
            if p16:
                p = p.to(dtype).to(f32)
            l = l * alpha + p.sum(-1)
            acc = acc * alpha[..., None] + torch.matmul(p, v[:, a:e])
            m = m_new
        live = l > 0
        o = acc / torch.where(live, l, torch.ones_like(l))[..., None]
        out[b] = torch.where(live[..., None], o, torch.zeros_like(o)).to(dtype)
    return out


# ---- hostile caches -------------------------------------------------------------------------------------------------
def quantise(x, scale):
    """The cache-write formula: e4m3fn(clamp(x * (1 / scale), -448, 448)), x fp32."""
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(scale), dtype=torch.float32)
    return (x.float() * inv).clamp(-448, 448).to(F8)


def nan_cache(shape, cache_dtype):
    if cache_dtype == F8:
        return torch.full(shape, F8_NAN, dtype=torch.uint8).view(F8)
    return torch.full(shape, float("nan"), dtype=cache_dtype)


def hostile_cache(ctxs, *, block_size, Hkv, D, L, layer, cache_dtype, gen, max_blocks=None, fill=None, k_scale=1.0,
                  v_scale=1.0, spare_blocks=3):
    """(k_cache, v_cache, block_tables [B,max_blocks] int32, nan_block) on the CPU for sequences of ctxs keys.

    fill(b, n) -> (k, v) fp32 [n, Hkv, D]: the values of sequence b's n = min(ctx, max_blocks * block_size) owned keys
    (default randn); an fp8 cache stores quantise(value, scale).  Physical blocks are a random permutation; sequences
    own disjoint blocks; `spare_blocks` blocks are owned by nobody.  Everything else is NaN (see the module docstring).
    max_blocks defaults to one more than the longest sequence needs."""
    bs = int(block_size)
    need_all = [(int(c) + bs - 1) // bs for c in ctxs]
    if max_blocks is None:
        max_blocks = max(need_all + [0]) + 1
    need = [min(x, max_blocks) for x in need_all]
    nb = sum(need) + spare_blocks + 1
    perm = torch.randperm(nb, generator=gen)
    nan_block = int(perm[0])
    bt = torch.full((len(ctxs), max_blocks), nan_block, dtype=torch.int32)
    kc = nan_cache((nb, L, bs, Hkv, D), cache_dtype)
    vc = nan_cache((nb, L, bs, Hkv, D), cache_dtype)
    at = 1
    for b, c in enumerate(ctxs):
        bt[b, :need[b]] = perm[at:at + need[b]].to(torch.int32)
        at += need[b]
        n = seq_len_eff(c, max_blocks, bs)
        if n == 0:
            continue
        if fill is None:
            k, v = torch.randn(n, Hkv, D, generator=gen), torch.randn(n, Hkv, D, generator=gen)
        else:
            k, v = fill(b, n)
        pos = torch.arange(n)
        blk, slot = bt[b, pos // bs].long(), pos % bs
        if cache_dtype == F8:
            kc[blk, layer, slot] = quantise(k, k_scale)
            vc[blk, layer, slot] = quantise(v, v_scale)
        else:
            kc[blk, layer, slot] = k.to(cache_dtype)
            vc[blk, layer, slot] = v.to(cache_dtype)
    return kc, vc, bt, nan_block


def is_nan_slots(cache):
    """[num_blocks, L, block_size] bool: slots that are NaN in every element (fp8: every byte 0x7f)."""
    if cache.dtype == F8:
        return (cache.view(torch.uint8) == F8_NAN).all(-1).all(-1)
    return torch.isnan(cache).all(-1).all(-1)


# ---- the check ------------------------------------------------------------------------------------------------------
def row_errors(o, ref):
    """Per-row ||o - ref|| / ||ref|| ([B,H,q_len,D] both) as [B,H,q_len] fp64; rows whose reference is 0 count their
    absolute norm."""
    d = o.to("cpu", torch.float64) - ref
    rn = ref.norm(dim=-1)
    return d.norm(dim=-1) / torch.where(rn > 0, rn, torch.ones_like(rn))


def measure(o, ref, ref_lse, dtype):
    """dict(worst, mean, seq) in units of u over the live rows (those whose ref_lse is finite)."""
    live = ~(torch.isinf(ref_lse) & (ref_lse < 0))
    e = row_errors(o, ref) / U[dtype]
    e = torch.where(live, e, torch.zeros_like(e))
    n_live = max(int(live.sum()), 1)
    per_seq = e.flatten(1).sum(1) / live.flatten(1).sum(1).clamp_min(1)
    return {"worst": e.max().item(), "mean": e.sum().item() / n_live, "seq": per_seq.max().item()}


def bars(model_o, ref, ref_lse, dtype):
    ms = measure(model_o, ref, ref_lse, dtype)
    return {k: max(MARGINS[k] * ms[k], FLOOR) for k in MARGINS}, ms


def check(o, ref, ref_lse, dtype, family, model_o, what="", win=False):
    """Assert the kernel result o [B,H,q_len,D] matches the fp64 reference (ref, ref_lse) within the bars taken from
    model_o (model() on the same inputs).  family = (q dtype, route, cache kind); returns the measured statistics."""
    tag = f"{what} [{family[1]} {family[2]} {str(dtype).split('.')[-1]}]"
    o = o.detach().to("cpu")
    assert o.shape == ref.shape, f"{tag}: shape {tuple(o.shape)} vs {tuple(ref.shape)}"
    bad = ~torch.isfinite(o.float())
    assert not bad.any(), (f"{tag}: non-finite output ({int(bad.sum())} values, sequences "
                           f"{sorted(set(bad.nonzero()[:, 0].tolist()))[:8]})")
    empty = torch.isinf(ref_lse) & (ref_lse < 0)
    assert (o[empty] == 0).all(), f"{tag}: rows with no visible key are not exactly 0"
    st = measure(o, ref, ref_lse, dtype)
    bar, ms = bars(model_o, ref, ref_lse, dtype)
    rec = STATS.setdefault(tuple(family) + (bool(win),), {"n": 0, "ratio": 0.0, **{k: 0.0 for k in MARGINS},
                                                          **{"model_" + k: 0.0 for k in MARGINS}})
    rec["n"] += 1
    for k in MARGINS:
        rec[k] = max(rec[k], st[k])
        rec["model_" + k] = max(rec["model_" + k], ms[k])
        rec["ratio"] = max(rec["ratio"], st[k] / bar[k])
    if not all(st[k] <= bar[k] for k in MARGINS):
        e = row_errors(o, ref) / U[dtype]
        b, h, qi = (int(x) for x in (e == e.max()).nonzero()[0])
        per_seq = (e.flatten(1).sum(1) / (~empty).flatten(1).sum(1).clamp_min(1)).tolist()
        raise AssertionError(
            f"{tag}: worst row {st['worst']:.2f} u (bar {bar['worst']:.2f}, model {ms['worst']:.2f}) at sequence {b} "
            f"head {h} row {qi}; mean {st['mean']:.3f} u (bar {bar['mean']:.3f}, model {ms['mean']:.3f}); worst "
            f"sequence mean {st['seq']:.2f} u (bar {bar['seq']:.2f}, model {ms['seq']:.2f}); per-sequence means "
            f"{[round(x, 2) for x in per_seq]}")
    return st


def stats_table():
    """STATS as the lines of the module docstring's table."""
    lines = ["q dtype  route  cache  window |  kernel: worst   mean    seq  |  model: worst   mean    seq  | ratio   n"]
    for key in sorted(STATS, key=str):
        d, route, kind, win = key
        r = STATS[key]
        lines.append(f"{str(d).split('.')[-1]:8s} {route:6s} {kind:6s} {'yes' if win else 'no ':6s} |"
                     f"        {r['worst']:6.2f} {r['mean']:6.3f} {r['seq']:6.2f}  |"
                     f"       {r['model_worst']:6.2f} {r['model_mean']:6.3f} {r['model_seq']:6.2f}  | {r['ratio']:5.2f} {r['n']:3d}")
    return "\n".join(lines)


def old_aggregate(o, ref, dtype):
    """The whole-tensor verdict the decode tests used before (tests/test_gpu_kernels.py::_cmp): (rel, max, passed)."""
    rtol, atol = {torch.float16: (1e-3, 4e-3), torch.bfloat16: (3e-3, 2e-2)}[dtype]
    r = ref.to(dtype).float()
    g = o.float().cpu()
    rel = ((g - r).abs().mean() / r.abs().mean().clamp_min(1e-12)).item()
    mx = (g - r).abs().max().item()
    return rel, mx, bool(rel < rtol and mx < atol * max(1.0, r.abs().max().item()))


# ---- data kinds -----------------------------------------------------------------------------------------------------
NEEDLE_LEAD = 20.0   # the needle key's score above the rest
OFFSET = 40.0        # the common score of the offset kind


def needle_position(place, ctx, n, q_len, left):
    """Key index of the needle of a sequence with n existing keys (None: the sequence gets none)."""
    if n == 0:
        return None
    lo0 = max(0, int(ctx) - q_len - left) if left >= 0 else 0   # row 0's first visible key
    pos = {"first": 0, "last": int(ctx) - 1, "win_in": lo0, "win_out": lo0 - 1, "255": 255, "256": 256,
           "mid": int(ctx) // 2 + 3}[place]
    if pos < 0:
        return None
    return min(pos, n - 1)


def make_inputs(case, gen):
    """q [B,H,q_len,D] fp32 values (before rounding to the dtype) and the fill(b, n) of hostile_cache for a case's data
    kind.  randn: q x 1.5.  The other kinds draw q = c + 0.3 randn around one direction c per (sequence, kv head), so
    that a key proportional to c scores the same for every query that reads it:
      needle: one key a c / |c|^2 with a * scale = NEEDLE_LEAD, its V row 4 randn, at case["needle"];
      offset: K = k0 + 0.1 randn with k0 = a c / |c|^2, a * scale = OFFSET;   vmean: V = 1 + 0.05 randn."""
    B, H, Hkv, q_len, D = case["B"], case["H"], case["Hkv"], case["q_len"], case["D"]
    kind, left, ctxs = case["data"], case["left"], case["ctxs"]
    scale = 1.0 / math.sqrt(D)
    if kind in ("randn", "vmean"):
        q = torch.randn(B, H, q_len, D, generator=gen) * 1.5
        c = None
    else:
        c = torch.randn(B, Hkv, D, generator=gen)
        q = c.repeat_interleave(H // Hkv, dim=1)[:, :, None, :] + 0.3 * torch.randn(B, H, q_len, D, generator=gen)

    def fill(b, n):
        k = torch.randn(n, Hkv, D, generator=gen)
        v = torch.randn(n, Hkv, D, generator=gen)
        if kind == "vmean":
            v = 1.0 + 0.05 * v
        elif kind == "offset":
            k = 0.1 * k + (OFFSET / scale) * c[b] / c[b].square().sum(-1, keepdim=True)
        elif kind == "needle":
            at = needle_position(case["needle"], ctxs[b], n, q_len, left)
            if at is not None:
                k[at] = (NEEDLE_LEAD / scale) * c[b] / c[b].square().sum(-1, keepdim=True)
                v[at] = 4.0 * torch.randn(Hkv, D, generator=gen)
        return k, v

    return q, fill


# ---- the case table -------------------------------------------------------------------------------------------------
BF, FP = torch.bfloat16, torch.float16
BLOCK_SIZES = [16, 1, 64, 12, 256, 8]
GRAN = {"head": 32, "rows": 32, "gqa": 128}
_EXTRA_CTX = [300, 77, 1000, 640, 200, 950, 45, 700, 260, 820, 150, 990]

# (window, data kind, needle place) of the cases of every (route, cache kind) cell.  Windows: None; "0": left 0; "q": left
# q_len - 1 (below q_len); "37": inside the contexts, no multiple of 32 or of a block size; "c": left 1050 at max_seq_len
# 1100 (>= most contexts, still the windowed kernel); "l": left 1029 at max_seq_len 2100 (several splits inside the window)
_PLAN = [
    (None, "randn", None), (None, "needle", "first"), (None, "needle", "255"), (None, "needle", "256"),
    (None, "offset", None), (None, "vmean", None),
    ("0", "randn", None), ("0", "needle", "last"),
    ("q", "randn", None), ("q", "needle", "win_in"),
    ("37", "randn", None), ("37", "needle", "win_in"), ("37", "needle", "win_out"), ("37", "vmean", None),
    ("c", "randn", None), ("c", "offset", None),
    ("l", "randn", None), ("l", "needle", "win_out"), ("l", "needle", "mid"),
]

# geometries per (route, fp8): B, H, Hkv, D, q_len, out_pad (elements of padding behind each output row; 4 puts the rows 8
# bytes off 16-byte alignment, which keeps D 128 away from the matrix-core kernel)
_G = lambda B, H, Hkv, D, q_len=1, out_pad=None: dict(B=B, H=H, Hkv=Hkv, D=D, q_len=q_len, out_pad=out_pad)
_GEOMS = {
    ("head", False): [_G(12, 4, 2, 8), _G(10, 4, 2, 48, 3), _G(12, 4, 2, 80), _G(10, 4, 2, 96, 3), _G(12, 4, 2, 112),
                      _G(4, 32, 1, 128), _G(12, 4, 4, 64), _G(3, 8, 2, 64, 5), _G(12, 4, 4, 128, 1, 4),
                      _G(3, 8, 2, 128, 5), _G(4, 32, 1, 64)],
    ("head", True): [_G(12, 4, 2, 16), _G(10, 4, 2, 48, 3), _G(12, 4, 2, 80), _G(10, 4, 2, 96, 3), _G(12, 4, 2, 112),
                     _G(4, 32, 1, 128), _G(12, 4, 4, 64), _G(3, 8, 2, 64, 5), _G(12, 4, 4, 128, 1, 4),
                     _G(3, 8, 2, 128, 5)],
    ("rows", False): [_G(16, 2, 2, 64), _G(18, 8, 8, 64), _G(16, 16, 16, 64), _G(18, 32, 32, 64),
                      _G(16, 4, 4, 128, 1, 4), _G(18, 16, 16, 128, 1, 4)],
    ("rows", True): [_G(16, 4, 4, 64), _G(18, 16, 16, 64), _G(16, 64, 64, 64), _G(18, 4, 4, 128, 1, 4),
                     _G(16, 32, 32, 128, 1, 4)],
    ("gqa", False): [_G(12, 4, 4, 128), _G(12, 4, 2, 64), _G(3, 6, 2, 128), _G(12, 12, 2, 64), _G(1, 24, 2, 128),
                     _G(3, 16, 1, 64), _G(12, 2, 2, 128, 2), _G(3, 4, 4, 64, 3), _G(12, 4, 2, 128, 3),
                     _G(1, 8, 2, 64, 3), _G(3, 16, 2, 128, 2), _G(12, 32, 2, 64)],
    ("gqa", True): [_G(12, 4, 4, 128), _G(12, 4, 2, 64), _G(3, 6, 2, 128), _G(12, 12, 2, 64), _G(1, 24, 2, 128),
                    _G(3, 16, 1, 64), _G(12, 2, 2, 128, 2), _G(3, 4, 4, 64, 3), _G(12, 4, 2, 128, 3),
                    _G(1, 8, 2, 64, 3), _G(3, 16, 2, 128, 2), _G(12, 32, 2, 64)],
}


def edge_contexts(route, bs, msl, B, short_table, rnd):
    """B contexts for a batch: the edges of the route's granularity g, of the block size, of a multiple of 256, and
    max_seq_len; with short_table the block-table row holds cap < max_seq_len keys and the batch has contexts of cap,
    cap + 5 and cap + block_size keys.  A batch of three or more holds exactly one empty sequence, a smaller one none.
    Returns (contexts, max_blocks)."""
    g = GRAN[route]
    if short_table:
        max_blocks = (msl - max(bs, 5)) // bs
        cap = max_blocks * bs
        first = [cap + 5, cap, cap + bs, msl, 1, bs + 1, bs, bs - 1, g + 1, 513, g, g - 1, 512, 511]
    else:
        max_blocks = (msl + bs - 1) // bs + 1
        first = [msl, 1, bs + 1, bs, bs - 1, g, g - 1, g + 1, 513, 512, 511]
    want = []
    for c in first + _EXTRA_CTX:
        if c > 0 and c not in want:
            want.append(c)
    n = B - 1 if B >= 3 else B
    start = rnd.randrange(len(want)) if 3 <= B < 8 and not short_table else 0   # small batches take different edges
    ctxs = [want[(start + i) % len(want)] for i in range(n)]
    if B >= 3:
        ctxs.insert(rnd.randrange(B), 0)
    return ctxs, max_blocks


def _left_of(win, q_len):
    return {None: -1, "0": 0, "q": q_len - 1, "37": 37, "c": 1050, "l": 1029}[win]


def _build_cases():
    cases = []
    for (route, kv8), geoms in _GEOMS.items():
        rnd = random.Random(f"{route}{kv8}")
        plan = list(_PLAN) + [(None, "randn", None), ("37", "randn", None)]   # the last two: short block-table rows
        for i, (win, data, place) in enumerate(plan):
            geo = dict(geoms[i % len(geoms)])
            if win == "q" and route != "rows":   # a window shorter than q_len needs several query rows
                geo = dict(next(x for x in geoms[i % len(geoms):] + geoms if x["q_len"] > 1))
            bs = BLOCK_SIZES[(i + i // 6) % len(BLOCK_SIZES)]   # drifts against the geometry cycle
            msl = 2100 if win == "l" else 1100
            short = i >= len(_PLAN)
            if short:   # room for the contexts around the end of the row
                geo = dict(next(x for x in geoms[i % len(geoms):] + geoms if x["B"] >= 10))
            ctxs, max_blocks = edge_contexts(route, bs, msl, geo["B"], short, rnd)
            out_pad = geo.pop("out_pad")
            if out_pad is None:
                out_pad = 8 if i % 4 == 1 else 0   # a view into a wider buffer; 8 elements keep the rows 16-byte aligned
            cases.append(dict(name=f"{route}-{'fp8' if kv8 else 'kv16'}-{i:02d}", route=route, kv8=kv8,
                              dtype=(BF, FP)[(i + i // 8) % 2], bs=bs, left=_left_of(win, geo["q_len"]), msl=msl,
                              ctxs=ctxs, max_blocks=max_blocks, data=data, needle=place, q_packed=(i % 3 == 0),
                              out_pad=out_pad, equal_unwindowed=False, seed=1000 * len(cases) + i, **geo))
        # max_seq_len far above every context: most splits are empty
        geo = dict(geoms[1])
        out_pad = geo.pop("out_pad") or 0
        ctxs = [300, 0, 33, 257, 1, 129, 64, 299, 17, 250, 128, 100, 31, 200, 2, 290, 96, 77][:geo["B"]]
        cases.append(dict(name=f"{route}-{'fp8' if kv8 else 'kv16'}-msl32768", route=route, kv8=kv8, dtype=BF, bs=16,
                          left=-1, msl=32768, ctxs=ctxs, max_blocks=32768 // 16, data="randn", needle=None,
                          q_packed=False, out_pad=out_pad, equal_unwindowed=False, seed=7 + len(cases), **geo))
        # a window of max_seq_len + q_len or more is the unwindowed launch, bit for bit
        geo = dict(geoms[0])
        out_pad = geo.pop("out_pad") or 0
        ctxs, max_blocks = edge_contexts(route, 16, 1100, geo["B"], False, rnd)
        cases.append(dict(name=f"{route}-{'fp8' if kv8 else 'kv16'}-wide-window", route=route, kv8=kv8, dtype=FP, bs=16,
                          left=1100 + geo["q_len"], msl=1100, ctxs=ctxs, max_blocks=max_blocks, data="randn",
                          needle=None, q_packed=False, out_pad=out_pad, equal_unwindowed=True, seed=9 + len(cases),
                          **geo))
    # the matrix-core kernel's block-table slice at block size 1: dec_nsplit_gqa adds splits until a slice fits DG_BT_MAX
    for kv8 in (False, True):
        cases.append(dict(name=f"gqa-{'fp8' if kv8 else 'kv16'}-bt-slice", route="gqa", kv8=kv8, dtype=BF, bs=1, left=-1,
                          msl=8192, ctxs=[8192, 0, 4097, 8191, 2049, 1, 300, 128, 640, 127, 33, 2048],
                          max_blocks=8193, data="randn", needle=None, q_packed=False, out_pad=0, equal_unwindowed=False,
                          seed=31 + kv8, B=12, H=16, Hkv=8, D=128, q_len=1))
    return cases


CASES = _build_cases()


def _ws_case(name, route, kv8, *, B, H, Hkv, D, bs, ctxs, msl, left=-1, q_len=1, out_pad=0, dtype=BF):
    return dict(name=name, route=route, kv8=kv8, dtype=dtype, bs=bs, left=left, msl=msl, ctxs=ctxs,
                max_blocks=(msl + bs - 1) // bs + 1, data="randn", needle=None, q_packed=False, out_pad=out_pad,
                equal_unwindowed=False, seed=500 + len(name), B=B, H=H, Hkv=Hkv, D=D, q_len=q_len)


# launches through the C ABI with a workspace of exactly mio_fa3_decode_workspace_bytes(): each route and cache kind, block
# sizes 1 and 256, one kv head, one sequence with a long context, a window
WORKSPACE_CASES = [
    _ws_case("ws-head-kv16-hkv1-bs1", "head", False, B=4, H=32, Hkv=1, D=128, bs=1, ctxs=[2100, 0, 513, 1], msl=2100),
    _ws_case("ws-head-fp8-bs256-win", "head", True, B=12, H=4, Hkv=2, D=80, bs=256, left=1029, msl=2100,
             ctxs=[2100, 1, 0, 31, 32, 33, 255, 256, 257, 512, 1031, 2047]),
    _ws_case("ws-rows-kv16-bs256", "rows", False, B=16, H=8, Hkv=8, D=64, bs=256, msl=1100,
             ctxs=[1100, 1, 0, 31, 32, 33, 255, 256, 257, 512, 700, 1000, 64, 65, 300, 77], dtype=FP),
    _ws_case("ws-rows-fp8-bs1-win", "rows", True, B=18, H=16, Hkv=16, D=64, bs=1, left=1029, msl=2100,
             ctxs=[2100, 1, 0, 31, 32, 33, 255, 256, 257, 512, 700, 1000, 64, 65, 300, 77, 2099, 1031]),
    _ws_case("ws-gqa-kv16-b1-hkv1-bs1", "gqa", False, B=1, H=8, Hkv=1, D=128, bs=1, ctxs=[8192], msl=8192),
    _ws_case("ws-gqa-fp8-bs256", "gqa", True, B=3, H=6, Hkv=2, D=128, bs=256, ctxs=[1100, 0, 129], msl=1100, dtype=FP),
    _ws_case("ws-gqa-kv16-win", "gqa", False, B=12, H=4, Hkv=2, D=64, bs=16, left=1029, msl=2100,
             ctxs=[2100, 1, 0, 127, 128, 129, 255, 256, 257, 512, 1031, 2047]),
]


def case_strides(case):
    """(q strides, o strides) in elements over (b, h, s) as the GPU test lays the case out: q contiguous or the q third
    of a packed [B, q_len, 3, H, D] projection; o a view of a [B, H, q_len, D + out_pad] buffer."""
    H, q_len, D = case["H"], case["q_len"], case["D"]
    qs = (q_len * 3 * H * D, D, 3 * H * D) if case["q_packed"] else (H * q_len * D, q_len * D, D)
    Dp = D + case["out_pad"]
    return qs, (H * q_len * Dp, q_len * Dp, Dp)


def case_scales(case):
    """(k_scale, v_scale) lists over the L layers of a case's cache: [1.0] * L for a 16-bit cache; for fp8, values that
    are no powers of two, the tested layer's sized so that the data kind's largest values stay inside e4m3fn's range."""
    if not case["kv8"]:
        return [1.0] * case_layers(case), [1.0] * case_layers(case)
    lead = {"needle": NEEDLE_LEAD, "offset": OFFSET}.get(case["data"], 0.0)
    kmax = max(5.0, 8.0 * lead / math.sqrt(case["D"]))   # a key a c / |c|^2 has elements of about lead / sqrt(D)
    return [0.9, kmax / 416.0, 1.7], [1.3, 16.0 / 416.0, 0.47]


def case_layers(case):
    return 3 if case["kv8"] else 2


LAYER = 1


def build_case(case):
    """The CPU tensors of a case: dict(q [B,H,q_len,D] in dtype, kc, vc, bt, ctx, k_scale, v_scale (lists), nan_block)."""
    gen = torch.Generator().manual_seed(case["seed"])
    qv, fill = make_inputs(case, gen)
    ks, vs = case_scales(case)
    kc, vc, bt, nan_block = hostile_cache(
        case["ctxs"], block_size=case["bs"], Hkv=case["Hkv"], D=case["D"], L=case_layers(case), layer=LAYER,
        cache_dtype=F8 if case["kv8"] else case["dtype"], gen=gen, max_blocks=case["max_blocks"], fill=fill,
        k_scale=ks[LAYER], v_scale=vs[LAYER])
    return dict(q=qv.to(case["dtype"]), kc=kc, vc=vc, bt=bt, ctx=torch.tensor(case["ctxs"], dtype=torch.int32),
                k_scale=ks, v_scale=vs, nan_block=nan_block)


def case_reference(case, t):
    """(ref, ref_lse, model_o) of a built case."""
    kw = dict(left=case["left"], k_scale=t["k_scale"][LAYER], v_scale=t["v_scale"][LAYER])
    ref, lse = reference(t["q"], t["kc"], t["vc"], t["bt"], t["ctx"], case["bs"], LAYER, **kw)
    mo = model(t["q"], t["kc"], t["vc"], t["bt"], t["ctx"], case["bs"], LAYER, dtype=case["dtype"],
               p16=case["route"] == "gqa", **kw)
    return ref, lse, mo


def family(case):
    return (case["dtype"], case["route"], "fp8" if case["kv8"] else "kv16")
