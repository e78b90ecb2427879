"""No GPU: the case table of tests/conv_special_cases.py can fail.

Each kernel's INDEX ARITHMETIC is restated here in torch, values in fp32 in K
order (csrc/conv_stem.hip, conv_n1.hip, bottleneck.hip, optim.hip):

  * stem forward: tile -> (img, ho0, wo0); the 27 absolute 8-element chunks of
    each of the 21 staged rows from floor8(E) (chunk 0 substituted when a chunk
    is outside the tensor or its row outside the image); the pixel pass (row
    d = E mod 8, 3 elements -> the 4-channel padded pixel, zeros outside the
    image); the 8-element tap groups (taps 0..7 x channels 0..3, tap 7 zeroed
    in registers, zero weights for tap 7 and channel 3); the persistent tile
    loop with its prefetch; the guarded stores into a flat output;
  * stem weight gradient: persistent blocks over output rows, the 7 staged
    input rows, the pixel-pair build of T (second half zeroed at an odd wo,
    pad columns and the dz tail never written), block slabs summed in block
    order into dw += col_scale * sum;
  * single filter: pixel -> level by prefix -> (n, oh, ow); taps t / S, t % S;
    the forward's lanes and xor-tree; the bwd-data's weights staged from the
    flipped copy; the bwd-filter's per-block pixel ranges with dead pixels;
  * bottleneck: the padded grid of W + 2 columns, tile + halo rows, the nine
    shifted taps m + (t / 3) WP + t % 3, bf16 intermediates;
  * weight prep: the OHWI and flipped index maps.

Checked: the unmutated restatement is inside every bound and bit-exact on the
exact cases; the fp64 reference rounded to the output dtype passes and halving
the bf16 store term rejects it; the restated host predicates and grids
reproduce every case's recorded kernel and grid; every branch is claimed by a
case; n1_xcd_block is a bijection on [0, nb) for nb <= 2048; the stem
weight gradient's `w > 2 WP` guard is dead for pads 0..3 and w % 8 == 0; each
planted mutation leaves a bound or breaks an exact case.

Large cases are emulated at a reduced shape that keeps the branch (the stem's
persistent loop: 10 tiles on 8 blocks; the weight gradient's row loop: the
grid capped below the row count; the bottleneck: two images).

Mutations that no entry point can observe, proved dead here instead:
  * stem wgrad `odd_kept` (the second half of the last pixel pair kept at an
    odd wo) and `dz_tail` (the dz image's columns past wo holding the next
    row's data): each alone multiplies a zero of the other operand, so with
    finite data the result is bit-identical; the two together are caught;
  * bottleneck `mid_unrounded` (the intermediates kept in fp32): the bound is
    centred on the unrounded fp64 reference, so dropping a rounding moves the
    result towards it; shown to stay inside the bound, and it cannot touch the
    exact cases (their intermediates are bf16 integers);
  * stem forward `keep_tap7` with finite data (tap 7's weights are zero): it is
    caught only by the Inf case, which is why that case exists.
"""
import dataclasses
import math

import pytest
import torch

import conv_special_cases as T

BF16, F32, F64 = T.BF16, T.F32, T.F64


def _flat_out(numel, dtype):
    return torch.full((numel + T.GUARD,), T.SENTINEL, dtype=dtype)


def _judge(case, outs, ref=None):
    """-> list of failures of outs {key: flat buffer with GUARD after} against the case's reference."""
    ref = ref or T.reference(case)
    bad = []
    for key, (r, bnd) in ref.items():
        buf = outs[key]
        n = r.numel()
        if not bool((buf[n:] == T.SENTINEL).all()):
            bad.append(f"{key}: guard written")
        ok, ratio = T.compare(buf[:n].view(r.shape), r, bnd)
        if not ok:
            bad.append(f"{key}: ratio {ratio:.3g}")
        if key != "dw" and bool((buf[:n] == T.SENTINEL).any()):
            bad.append(f"{key}: unwritten")
    return bad


# ------------------------------------------------------------ table / routes
def test_recorded_routes_match_the_restated_predicates():
    for c in T.CASES:
        assert T.route(c) == (c.kernel, c.grid), (c.name, T.route(c), c.kernel, c.grid)
        assert c.note, c.name
    assert T.bneck_route(dataclasses.replace(T.BNECK[0], hw=28)) == ("unsupported", 0)


def test_every_branch_is_claimed():
    for fam, branches in T.BRANCHES.items():
        claimed = set()
        for c in T.CASES + T.WPREP:
            if c.family == fam:
                claimed |= set(c.claims)
        assert claimed == branches, (fam, branches - claimed, claimed - branches)
    # the branch conditions themselves, from the geometry
    by = T.BY_NAME
    c = by["sf_misaligned_rows"]
    assert (3 * c.w) % 8 == 7 and (c.h * c.w * 3) % 8 == 7 and 3 * (0 - c.pads[2]) < 0
    c = by["sf_nopad_two_col_tiles"]
    assert (3 * c.w) % 8 == 1 and c.out_hw[1] == 35
    c = by["sf_asym_k128"]
    assert c.out_hw[0] == 9 and c.k == 128
    c = by["sf_persistent"]
    assert c.n * 1 * 1 == 1000 > c.grid == 768 and c.w < 69
    for name, rows, wo, wp in (("sw_two_rows", 520, 8, 16), ("sw_odd_wo", 335, 5, 16), ("sw_256_two_rows", 264, 116, 128),
                               ("sw_last_112", 16, 112, 112), ("sw_widest", 5, 256, 256), ("sw_pad_cols", 6, 17, 32)):
        c = by[name]
        assert (c.n * c.out_hw[0], c.out_hw[1], T.cdiv(c.out_hw[1], 16) * 16) == (rows, wo, wp), name
    c = by["n1_fwd_grid_cap"]
    P = T.n1_pixels(c)
    rounds = T.cdiv(P, 64)
    assert T.cdiv(rounds, c.grid) == 2 and (P % 128) != 0
    c = by["n1_bwd_filter_grid_cap"]
    assert T.n1_pixels(c) > 16384 and c.grid % 8
    assert T.n1_pixels(by["n1_bwd_filter_one_block"]) < 16


def n1_xcd_block(b, nb):
    q, r, x = nb >> 3, nb & 7, b & 7
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + (b >> 3)


def test_xcd_block_is_a_bijection():
    for nb in range(1, 2049):
        assert sorted(n1_xcd_block(b, nb) for b in range(nb)) == list(range(nb)), nb


def test_stem_wgrad_width_guard_is_dead():
    """d->w > 2 WP cannot hold once w % 8 == 0, pads in 0..3 and 2 wo <= 512 passed."""
    for w in range(8, 520, 8):
        for pl in range(4):
            for pr in range(4):
                wo = T.conv_out(w, pl, pr, 7, 2)
                if wo <= 0 or 2 * wo > 512 or w > 512:
                    continue
                wp = T.cdiv(wo, 16) * 16
                assert wp <= 256 and w <= 2 * wp, (w, pl, pr)


# --------------------------------------------- rounded reference / store term
STORE_CASES = ["sf_misaligned_rows", "sf_asym_k128", "sf_epi_leaky_scale", "n1_fwd_bf16_cv8", "n1_bwd_data_bf16_cv8",
               "n1_bwd_data_bf16_cv128", "n1_bwd_data_1x3"]


def test_rounded_reference_passes_every_bound():
    for c in T.CASES:
        for key, (r, bnd) in T.reference(c).items():
            od = F32 if key == "dw" else c.dtype
            ok, ratio = T.compare(r.to(od), r, bnd)
            assert ok and ratio <= 1, (c.name, key, ratio)


@pytest.mark.parametrize("name", STORE_CASES)
def test_half_the_store_term_rejects_the_rounded_reference(name, monkeypatch):
    monkeypatch.setattr(T, "U_STORE", 2.0 ** -9)
    c = T.BY_NAME[name]
    rejected = False
    for key, (r, bnd) in T.reference(c).items():
        ok, _ = T.compare(r.to(c.dtype), r, bnd)
        rejected |= not ok
    assert rejected, "the rounded reference passes with half the store term: the term is slack"


# ===================================================== stem forward, restated
def emu_stem_fwd(c, inp, mut=None, grid=None):
    x = inp["x"].float().reshape(-1)
    total = x.numel()
    k, h, wd = c.k, c.h, c.w
    W3 = 3 * wd
    ho, wo = c.out_hw
    tiles_h, tiles_w = T.cdiv(ho, 8), T.cdiv(wo, 32)
    tiles = c.n * tiles_h * tiles_w
    grid = grid or min(tiles, 768)
    pt, pl = c.pads[0], c.pads[2]
    if mut == "swap_pt_pl":
        pt, pl = pl, pt
    wreg = torch.zeros(k, 7, 8, 4)
    wreg[:, :, :7, :3] = inp["w"].float()  # tap 7 and channel 3: zero weights
    if mut == "chunk2_w":
        wreg[64:] = wreg[:64].repeat(k // 64 - 1, 1, 1, 1)
    scale = inp["scale"].float() if c.scale else None
    bias = inp["bias"].float() if c.bias else torch.zeros(k)
    y = _flat_out(c.n * ho * wo * k, BF16)
    hh, ci, e8, px = torch.arange(21), torch.arange(27), torch.arange(8), torch.arange(69)

    def coords(t):
        wo0 = (t % tiles_w) * 32
        t //= tiles_w
        return t // tiles_h, (t % tiles_h) * 8, wo0

    def prefetch(t):
        img, ho0, wo0 = coords(t)
        hi = 2 * ho0 - pt + hh
        row_ok = (hi >= 0) & (hi < h)
        E = (img * h + hi) * W3 + 3 * (2 * wo0 - pl)
        base = torch.div(E, 8, rounding_mode="trunc" if mut == "trunc_E" else "floor") * 8
        cs = base[:, None] + 8 * ci[None]
        ok = row_ok[:, None] & (cs >= 0) & (cs + 8 <= total)
        idx = torch.where(ok, cs, torch.zeros((), dtype=cs.dtype))[:, :, None] + e8
        return x[idx].reshape(21, 216), ok

    for b in range(grid):
        pf = None
        for tile in range(b, tiles, grid):
            if pf is None or mut != "stale_tile":
                pf = prefetch(tile)
            craw, chunk_ok = pf
            img, ho0, wo0 = coords(tile)
            rowm = (img * h + 2 * ho0 - pt) * W3 + 3 * (2 * wo0 - pl)
            d = (rowm + hh * W3) & 7
            if mut == "row_d0":
                d = torch.full_like(d, rowm & 7)
            src = d[:, None] + 3 * px[None]
            vals = torch.stack([craw[hh[:, None], src + ch] for ch in range(3)], -1)
            hi, wi = 2 * ho0 - pt + hh, 2 * wo0 - pl + px
            ok = ((hi >= 0) & (hi < h))[:, None] & ((wi >= 0) & (wi < wd) if mut != "mask_row_only" else wi == wi)[None]
            if mut == "chunk_leak":
                ok = ok | ~chunk_ok[hh[:, None], src // 8]
            raw = torch.zeros(21, 70, 4)
            raw[:, :69, :3] = torch.where(ok[..., None], vals, torch.zeros(()))
            rows = 2 * torch.arange(8)[:, None] + torch.arange(7)[None]      # [lrow][r]
            cols = 2 * torch.arange(32)[:, None] + torch.arange(8)[None]     # [nl][tap]
            P = raw[rows][:, :, cols]                                        # [lrow][r][nl][tap][ch]
            if mut != "keep_tap7":
                P[:, :, :, 7, :] = 0
            acc = torch.zeros(8, 32, k)
            for r in range(7):
                for sx in range(8):
                    for ch in range(4):
                        acc = acc + P[:, r, :, sx, ch][..., None] * wreg[:, r, sx, ch]
            v = acc * scale if scale is not None else acc
            v = T._act(v + bias, c.act).to(BF16)
            for j in range(8):
                for p in range(32):
                    row_in = ho0 + j <= ho if mut == "edge_le" else ho0 + j < ho
                    col_in = wo0 + p <= wo if mut == "edge_le" else wo0 + p < wo
                    if row_in and col_in:
                        o = ((img * ho + ho0 + j) * wo + wo0 + p) * k
                        if o + k <= y.numel():
                            y[o:o + k] = v[j, p]
    return {"y": y}


def _small(c):
    """The reduced shape of a large stem-forward case and its grid."""
    if c.name == "sf_persistent":
        return dataclasses.replace(c, n=10), 8
    return c, None


SF_EMU = ["sf_pt_ne_pl", "sf_misaligned_rows", "sf_nopad_two_col_tiles", "sf_asym_k128", "sf_persistent", "sf_epi_relu_scale_bias",
          "sf_epi_leaky_scale", "sf_exact", "sf_inf"]


@pytest.mark.parametrize("name", SF_EMU)
def test_stem_fwd_restatement_is_inside_the_bound(name):
    c, grid = _small(T.BY_NAME[name])
    inp = T.inputs(c)
    bad = _judge(c, emu_stem_fwd(c, inp, grid=grid), T.reference(c, inp))
    assert not bad, bad


SF_MUT = [("row_d0", "sf_misaligned_rows"), ("trunc_E", "sf_misaligned_rows"), ("swap_pt_pl", "sf_pt_ne_pl"),
          ("mask_row_only", "sf_misaligned_rows"), ("keep_tap7", "sf_inf"), ("chunk_leak", "sf_inf"),
          ("chunk2_w", "sf_asym_k128"), ("chunk2_w", "sf_exact"), ("edge_le", "sf_misaligned_rows"),
          ("stale_tile", "sf_persistent"), ("swap_pt_pl", "sf_exact"), ("mask_row_only", "sf_exact")]


@pytest.mark.parametrize("mut,name", SF_MUT)
def test_stem_fwd_mutation_is_caught(mut, name):
    c, grid = _small(T.BY_NAME[name])
    inp = T.inputs(c)
    assert _judge(c, emu_stem_fwd(c, inp, mut, grid), T.reference(c, inp)), f"{mut} passes on {name}"


def test_stem_fwd_tap7_is_hidden_by_finite_data():
    """Why the Inf case exists: with finite data tap 7 meets zero weights."""
    c = T.BY_NAME["sf_misaligned_rows"]
    inp = T.inputs(c)
    assert torch.equal(emu_stem_fwd(c, inp, "keep_tap7")["y"], emu_stem_fwd(c, inp)["y"])


# ============================================== stem weight gradient, restated
def emu_stem_wgrad(c, inp, muts=(), grid=None):
    x = inp["x"].float()
    dz = inp["dz"].float()
    n, h, wd = c.n, c.h, c.w
    ho, wo = c.out_hw
    pt, pl = c.pads[0], c.pads[2]
    WP = 112 if T.cdiv(wo, 16) * 16 <= 112 else 256
    rows = n * ho
    grid = grid or min(rows, 512 if WP == 112 else 256)
    dzf = dz.reshape(rows, wo, 64)
    slabs = []
    m = torch.arange(147)
    rs, ch = m // 3, m % 3
    r, sx = rs // 7, rs % 7
    npair = (wo + 1) >> 1
    pcol = torch.arange(2 * npair)        # the columns the pair writes cover
    for b in range(grid):
        tt = torch.zeros(160, WP + 8)     # zeroed once: pad rows and pad columns
        dzi = torch.zeros(WP, 64)
        acc = torch.zeros(147, 64)
        for t in range(b, rows, grid):
            img, oh = t // ho, t % ho
            xr = torch.zeros(7, wd, 3)
            for rr in range(7):
                hi = 2 * oh - pt + rr
                if 0 <= hi < h:
                    xr[rr] = x[img, hi]
            dzi[:wo] = dzf[t]
            if "dz_tail" in muts and t + 1 < rows:
                dzi[wo:min(WP, 2 * wo)] = dzf[t + 1][:min(WP, 2 * wo) - wo]
            col = 2 * pcol[None] - pl + sx[:, None]                      # [147][2 npair]
            inside = (col >= 0) & (col < wd)
            live = pcol[None] < wo if "odd_kept" not in muts else pcol[None] >= 0
            val = xr[r[:, None], col.clamp(0, wd - 1), ch[:, None]]
            tt[:147, :2 * npair] = torch.where(inside & live, val, torch.zeros(()))
            for kcol in range(WP):                                       # K order: one pixel at a time
                acc = acc + tt[:147, kcol][:, None] * dzi[kcol][None]
        slabs.append(acc)
    tot = torch.zeros(147, 64)
    for s in slabs:
        tot = tot + s
    if c.col_scale and "no_scale" not in muts:
        tot = tot * inp["col_scale"].float()
    old = inp["old"].float().reshape(147, 64)
    out = _flat_out(147 * 64, F32)
    out[:147 * 64] = (tot if "assign" in muts else old + tot).reshape(-1)
    return {"dw": out}


def _small_sw(c):
    """Reduced shapes: few images, the grid capped under the row count so the
    row loop and its re-staging still run."""
    red = {"sw_two_rows": (3, 20), "sw_odd_wo": (3, 8), "sw_256_two_rows": (2, 12), "sw_256_asym": (2, 12),
           "sw_last_112": (1, 8), "sw_widest": (1, 5), "sw_pad_cols": (3, 6), "sw_exact": (65, 512)}[c.name]
    return dataclasses.replace(c, n=red[0]), red[1]


@pytest.mark.parametrize("name", ["sw_two_rows", "sw_odd_wo", "sw_256_asym", "sw_last_112", "sw_pad_cols", "sw_exact"])
def test_stem_wgrad_restatement_is_inside_the_bound(name):
    c, grid = _small_sw(T.BY_NAME[name])
    inp = T.inputs(c)
    bad = _judge(c, emu_stem_wgrad(c, inp, grid=grid), T.reference(c, inp))
    assert not bad, bad


@pytest.mark.parametrize("muts,name", [(("odd_kept", "dz_tail"), "sw_odd_wo"), (("assign",), "sw_two_rows"),
                                       (("assign",), "sw_exact"), (("no_scale",), "sw_odd_wo")])
def test_stem_wgrad_mutation_is_caught(muts, name):
    c, grid = _small_sw(T.BY_NAME[name])
    inp = T.inputs(c)
    assert _judge(c, emu_stem_wgrad(c, inp, muts, grid), T.reference(c, inp)), f"{muts} passes on {name}"


@pytest.mark.parametrize("mut", ["odd_kept", "dz_tail"])
def test_stem_wgrad_single_pad_mutations_are_dead(mut):
    """Alone, each meets a zero of the other operand: bit-identical results."""
    c, grid = _small_sw(T.BY_NAME["sw_odd_wo"])
    inp = T.inputs(c)
    assert torch.equal(emu_stem_wgrad(c, inp, (mut,), grid)["dw"], emu_stem_wgrad(c, inp, (), grid)["dw"])


def test_stem_wgrad_dz_swizzle_slot():
    """The dz row's 16-B chunk j of pixel wo is written to slot
    j ^ (((wo >> 1) & 1) << 2) of its 128-B row; the transposing read of pixel
    row kk, channel col computes the same slot: every (pixel, channel) is read
    back from where it was written, and without the xor on the read the pixels
    with (kk >> 1) & 1 set are not."""
    WP = 256
    where = {}
    for wo in range(WP):
        for j in range(8):
            for e in range(8):
                where[wo * 128 + ((j ^ (((wo >> 1) & 1) << 2)) << 4) + 2 * e] = (wo, 8 * j + e)
    assert len(where) == WP * 64

    def addr(kk, col, xor=True):
        return kk * 128 + ((((col >> 3) ^ ((((kk >> 1) & 1) << 2) if xor else 0)) << 4) | ((col & 7) << 1))
    assert all(where[addr(kk, col)] == (kk, col) for kk in range(WP) for col in range(64))
    assert any(where[addr(kk, col, False)] != (kk, col) for kk in range(4) for col in range(64))


# ===================================================== single filter, restated
def _n1_table(c, out_grid):
    """n1_args: the live levels, their first pixels (output grid for the forward, input grid else)."""
    lv, p = [], 0
    for i, (n, h, w) in enumerate(c.levels):
        ho, wo = c.out_hw(h, w)
        if n <= 0 or h <= 0 or w <= 0 or ho <= 0 or wo <= 0:
            continue
        lv.append(dict(i=i, n=n, H=h, W=w, Ho=ho, Wo=wo, p0=p))
        p += n * ho * wo if out_grid else n * h * w
    return lv, p


def _n1_level(lv, p, mut):
    L = lv[0]
    for cand in lv[1:]:
        if (p > cand["p0"]) if mut == "prefix_off_by_one" else (p >= cand["p0"]):
            L = cand
    return L


def _tap(t, c, mut):
    return (t // c.r, t % c.r) if mut == "tap_by_R" else (t // c.s, t % c.s)


def emu_n1(c, inp, mut=None):
    vn = 8 if c.dtype == BF16 else 4
    C, cv, taps = c.c, c.c // vn, c.r * c.s
    pt, pl = c.pads[0], c.pads[2]
    w = inp["w"].float().reshape(taps, C)
    xs, dzs = [t.float() for t in inp["xs"]], [t.float() for t in inp["dzs"]]
    outs = {}
    if c.op == "fwd":
        lv, P = _n1_table(c, True)
        for L in lv:
            outs[f"y{L['i']}"] = _flat_out(L["n"] * L["Ho"] * L["Wo"], c.dtype)
        lpp = min(cv, 64)
        nch = cv // lpp
        sc = float(inp["scale"].float()) if c.scale else None
        bi = inp["bias"].float()[0] if c.bias else torch.zeros(())
        for p in range(P):
            L = _n1_level(lv, p, mut)
            q = p - L["p0"]
            hw = L["Ho"] * L["Wo"]
            n, rem = q // hw, q % hw
            oh, ow = rem // L["Wo"], rem % L["Wo"]
            x = xs[L["i"]]
            acc = torch.zeros(lpp)
            for t in range(taps):
                dr, dc = _tap(t, c, mut)
                ih, iw = oh + dr - pt, ow + dc - pl
                if not (0 <= n < L["n"] and 0 <= ih < L["H"] and 0 <= iw < L["W"]):
                    continue
                prod = (x[n, ih, iw] * w[t]).view(nch, lpp, vn)
                for kk in range(nch):
                    for e in range(vn):
                        acc = acc + prod[kk, :, e]
            o = lpp // 2
            while o > (1 if mut == "lane_partner" else 0):
                acc = acc + acc[torch.arange(lpp) ^ o]
                o //= 2
            v = acc[0] * sc if sc is not None else acc[0]
            v = T._act(v + bi, c.act)
            buf = outs[f"y{L['i']}"]
            if 0 <= q < buf.numel() - T.GUARD:
                buf[q] = v.to(c.dtype)
        return outs
    lv, P = _n1_table(c, False)
    if c.op == "bwd_data":
        wflip = T._flip_of(inp["w"]).float().reshape(C, taps)      # w_flip[c][taps - 1 - t]
        ws = torch.zeros(taps, C)
        for tf in range(taps):
            ws[tf if mut == "unflipped" else taps - 1 - tf] = wflip[:, tf]
        for L in lv:
            outs[f"dx{L['i']}"] = _flat_out(L["n"] * L["H"] * L["W"] * C, c.dtype)
        for p in range(P):
            L = _n1_level(lv, p, mut)
            q = p - L["p0"]
            hw = L["H"] * L["W"]
            n, rem = q // hw, q % hw
            ih, iw = rem // L["W"], rem % L["W"]
            dz = dzs[L["i"]].reshape(-1)
            img = n * (L["H"] * L["W"] if mut == "stride_H" else L["Ho"] * L["Wo"])
            acc = torch.zeros(C)
            for t in range(taps):
                dr, dc = _tap(t, c, mut)
                oh, ow = ih - dr + pt, iw - dc + pl
                if 0 <= oh < L["Ho"] and 0 <= ow < L["Wo"]:
                    j = img + oh * L["Wo"] + ow
                    g = dz[j] if j < dz.numel() else torch.zeros(())
                    acc = acc + g * ws[t]
            if c.mask:
                yin = inp["ys"][L["i"]].float().reshape(-1, C)
                acc = acc * (yin[q] > 0).float() if q < yin.shape[0] else acc
            buf = outs[f"dx{L['i']}"]
            if (q + 1) * C <= buf.numel() - T.GUARD:
                buf[q * C:(q + 1) * C] = acc.to(c.dtype)
        return outs
    # bwd-filter: blocks of ppb input pixels, PL pixel lanes, two pixels per round
    nb = min(1024, max(1, P // 16))
    ppb = T.cdiv(P, nb)
    nb = T.cdiv(P, ppb)
    PL = 256 // cv
    tot = torch.zeros(taps, C)
    for vb in range(nb):
        pb, pe = vb * ppb, min(P, (vb + 1) * ppb)
        part = torch.zeros(taps, C)
        for lane in range(PL):
            for p0 in range(pb + lane, pe, 2 * PL):
                for u in range(2):
                    p = p0 + u * PL
                    if p >= pe:
                        if mut != "dead_pixel":
                            continue
                        p = pb  # the dead lane's clamped pixel, its product kept
                    L = _n1_level(lv, p, mut)
                    q = p - L["p0"]
                    hw = L["H"] * L["W"]
                    n, rem = q // hw, q % hw
                    ih, iw = rem // L["W"], rem % L["W"]
                    xf = xs[L["i"]].reshape(-1, C)
                    if q >= xf.shape[0]:
                        continue
                    dz = dzs[L["i"]].reshape(-1)
                    for t in range(taps):
                        dr, dc = _tap(t, c, mut)
                        oh, ow = ih - dr + pt, iw - dc + pl
                        if 0 <= oh < L["Ho"] and 0 <= ow < L["Wo"]:
                            part[t] = part[t] + xf[q] * dz[n * L["Ho"] * L["Wo"] + oh * L["Wo"] + ow]
        tot = tot + part
    out = _flat_out(taps * C, F32)
    out[:taps * C] = (inp["old"].float().reshape(taps, C) + tot).reshape(-1)
    return {"dw": out}


N1_EMU = [f"n1_{op}_{nm}" for op in ("fwd", "bwd_data", "bwd_filter")
          for nm in ("bf16_cv8", "f32_cv8", "bf16_cv128", "valid3x3", "1x3", "3x1", "2x2", "levels_mix", "exact")]
N1_EMU += ["n1_fwd_epi_leaky_scale", "n1_bwd_data_mask", "n1_bwd_filter_one_block"]


@pytest.mark.parametrize("name", N1_EMU)
def test_n1_restatement_is_inside_the_bound(name):
    c = T.BY_NAME[name]
    inp = T.inputs(c)
    bad = _judge(c, emu_n1(c, inp), T.reference(c, inp))
    assert not bad, bad


N1_MUT = [("tap_by_R", "n1_fwd_1x3"), ("tap_by_R", "n1_bwd_data_3x1"), ("tap_by_R", "n1_bwd_filter_1x3"),
          ("unflipped", "n1_bwd_data_bf16_cv8"), ("unflipped", "n1_bwd_data_exact"),
          ("prefix_off_by_one", "n1_fwd_levels_mix"), ("prefix_off_by_one", "n1_bwd_data_levels_mix"),
          ("prefix_off_by_one", "n1_bwd_filter_exact"), ("stride_H", "n1_bwd_data_valid3x3"),
          ("dead_pixel", "n1_bwd_filter_bf16_cv8"),
          ("dead_pixel", "n1_bwd_filter_exact"), ("lane_partner", "n1_fwd_bf16_cv8"), ("lane_partner", "n1_fwd_exact")]


@pytest.mark.parametrize("mut,name", N1_MUT)
def test_n1_mutation_is_caught(mut, name):
    c = T.BY_NAME[name]
    inp = T.inputs(c)
    assert _judge(c, emu_n1(c, inp, mut), T.reference(c, inp)), f"{mut} passes on {name}"


# ========================================================= bottleneck, restated
def emu_bneck(c, inp, mut=None):
    """Two images (base[0], base[-1]) through the padded-grid tile walk."""
    H = W = c.hw
    C, CM, TR = c.c, c.cm, c.tr
    WP = W + 2
    MB = 128
    MA = ((MB - 1 + 2 * WP + 2 + 1 + 63) // 64) * 64
    MA_VALID, MB_VALID = (TR + 2) * WP, TR * WP
    base = inp["base"]
    x = torch.stack([base[0], base[-1]]).float()
    n = 2
    xf = x.reshape(n * H, W, C)                      # image rows, flat over images
    wa, wc = inp["wa"].float(), inp["wc"].float()
    w3 = inp["w3"].float().reshape(CM, 9, CM)
    ba, b3, bc = inp["ba"].float(), inp["b3"].float(), inp["bc"].float()
    rnd = (lambda t: t) if mut == "mid_unrounded" else (lambda t: t.to(BF16).float())
    y = torch.full((n, H, W, C), T.SENTINEL)
    q = torch.arange(MA)
    mrow = torch.arange(MB)
    for img in range(n):
        for h0 in range(0, H, TR):
            hh = h0 - 1 + q // WP + (1 if mut == "seam_off_by_one" else 0)
            ww = q % WP - 1
            col_ok = (ww >= 0) & (ww < W)
            row_ok = (hh >= 0) & (hh < H)
            flat = img * H + hh
            if mut == "clamp":
                src_ok = (q < MA_VALID) & col_ok
                flat = img * H + hh.clamp(0, H - 1)
            elif mut == "neighbour_halo":
                src_ok = (q < MA_VALID) & col_ok & (flat >= 0) & (flat < n * H)
            else:
                src_ok = (q < MA_VALID) & col_ok & row_ok
            xa = torch.where(src_ok[:, None], xf[flat.clamp(0, n * H - 1), ww.clamp(0, W - 1)], torch.zeros(()))
            m1 = torch.where(src_ok[:, None], rnd((xa @ wa.t() + ba).clamp_min(0)), torch.zeros(()))
            m1 = torch.cat([m1, torch.zeros(2 * WP + 3, CM)])
            acc = torch.zeros(MB, CM)
            for t in range(9):
                if mut == "drop_tap" and t == 8:
                    continue
                acc = acc + m1[mrow + (t // 3) * WP + t % 3] @ w3[:, t, :].t()
            m2 = rnd((acc + b3).clamp_min(0))
            oh, ow = h0 + mrow // WP, mrow % WP
            ok = (mrow < MB_VALID) & (ow < W)
            res = torch.where(ok[:, None], x[img, oh.clamp(0, H - 1), ow.clamp(0, W - 1)], torch.zeros(()))
            if mut == "no_residual":
                res = torch.zeros_like(res)
            out = (m2 @ wc.t() + bc + res).clamp_min(0).to(BF16).float()
            y[img, oh[ok], ow[ok]] = out[ok]
    return y


def _bneck_ref2(c, inp):
    ref, bnd = T.bneck_reference(dataclasses.replace(c, n=c.uniq), inp)["y"]
    pick = [0, c.uniq - 1]
    return ref[pick], None if bnd is None else bnd[pick]


@pytest.mark.parametrize("name", [c.name for c in T.BNECK if c.n > 1])
def test_bottleneck_restatement_is_inside_the_bound(name):
    c = T.BY_NAME[name]
    inp = T.inputs(c)
    ref, bnd = _bneck_ref2(c, inp)
    ok, ratio = T.compare(emu_bneck(c, inp), ref, bnd)
    assert ok, ratio


BN_MUT = ["drop_tap", "clamp", "neighbour_halo", "seam_off_by_one", "no_residual"]


@pytest.mark.parametrize("mut", BN_MUT)
@pytest.mark.parametrize("name", ["bn_res2_exact", "bn_res3_exact"])
def test_bottleneck_mutation_breaks_the_exact_case(mut, name):
    c = T.BY_NAME[name]
    inp = T.inputs(c)
    ref, _ = _bneck_ref2(c, inp)
    assert not torch.equal(emu_bneck(c, inp, mut).double(), ref), f"{mut} passes on {name}"


@pytest.mark.parametrize("name", ["bn_res2_n10", "bn_res2_exact"])
def test_bottleneck_unrounded_mid_is_not_observable(name):
    """Proved unobservable: the bound's centre is the unrounded reference."""
    c = T.BY_NAME[name]
    inp = T.inputs(c)
    ref, bnd = _bneck_ref2(c, inp)
    ok, _ = T.compare(emu_bneck(c, inp, "mid_unrounded"), ref, bnd)
    assert ok


# ======================================================== weight prep, restated
def emu_wprep(c, inp, mut=None):
    """The kernels' element maps, one element at a time."""
    r, s, ci, k = c.shape
    w = inp["w"]
    sc = inp.get("scale")
    rs = r * s
    ldf = rs * k + c.ld_extra if c.ld_extra and mut != "ld_ignored" else rs * k
    ohwi = torch.full((k * rs * ci,), T.SENTINEL, dtype=c.dtype)
    flip = torch.full((ci * ldf,), T.SENTINEL, dtype=c.dtype)
    for rr in range(r):
        for ss in range(s):
            rsi = rr * s + ss
            for cc in range(ci):
                f = sc[torch.arange(k)] if sc is not None else torch.ones(k)
                if mut == "scale_by_c" and sc is not None:
                    f = sc[cc % k].expand(k)
                v = (w[rr, ss, cc] * f).to(c.dtype)
                ohwi[(torch.arange(k) * rs + rsi) * ci + cc] = v
                fr, fs = (rr, ss) if mut == "no_flip" else (r - 1 - rr, s - 1 - ss)
                o = cc * ldf + (fr * s + fs) * k
                flip[o:o + k] = v
    return ohwi, flip


@pytest.mark.parametrize("name", [c.name for c in T.WPREP if c.dtype == BF16])
def test_wprep_restatement_equals_the_expected_bits(name):
    c = T.BY_NAME[name]
    inp = T.inputs(c)
    o, f = emu_wprep(c, inp)
    eo, ef = T.wprep_expected(c, inp)
    assert torch.equal(o.view(torch.int16), eo.view(torch.int16)) and torch.equal(f.view(torch.int16), ef.view(torch.int16))


@pytest.mark.parametrize("mut,name", [("no_flip", "wp_bf16_3x3x33x65"), ("no_flip", "wp_bf16_1x3x40x36"),
                                      ("ld_ignored", "wp_bf16_k_not4"), ("scale_by_c", "wp_bf16_3x3x33x65"),
                                      ("scale_by_c", "wp_bf16_7x7x3x64")])
def test_wprep_mutation_is_caught(mut, name):
    c = T.BY_NAME[name]
    inp = T.inputs(c)
    o, f = emu_wprep(c, inp, mut)
    eo, ef = T.wprep_expected(c, inp)
    same = torch.equal(o.view(torch.int16), eo.view(torch.int16)) and f.numel() == ef.numel() and \
        torch.equal(f.view(torch.int16), ef.view(torch.int16))
    assert not same, f"{mut} passes on {name}"
    # and the table's own mutated expectation (what a GPU result with the error would be compared with) differs too
    mo, mf = T.wprep_expected(c, inp, mut)
    assert not (torch.equal(mo, eo) and mf.numel() == ef.numel() and torch.equal(mf, ef))
