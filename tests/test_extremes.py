"""Directed extreme-value inputs (tests/extremes.py): the host-side census and the reference pin.

CPU only.  A directed input that misses its target proves nothing, so for every family the census
asserts, from the inputs and the oracle alone, that the target is hit: blocks exactly at the packed
transforms' bound in packed waves and one past it in fallback waves, the 6-tap intermediates at their
extremes, every border crossed by every amount, every listed weight used, every designed deblocking
line filtered exactly as 8.7.2 says.  These are conditions, not measurements.

The GPU is compared with the oracle (tests/test_gpu_extremes.py); here the oracle is pinned to the
unmodified reference decoder on the same inputs: tests/golden/extremes.json holds the MD5s of what
the compiled reference made of each picture (tests/golden/make_extremes.py).
"""
import json
import os

import numpy as np
import pytest

import _oracle as O
import extremes as X
import extremes_d2 as D2
import extremes_i as I
import extremes_s as S
from h264r import _abi as A
from h264r import synth

_HERE = os.path.dirname(__file__)
EXT = json.load(open(os.path.join(_HERE, "golden", "extremes.json")))["cases"]
_IDS = [c["name"] for c in EXT]


@pytest.fixture(scope="module")
def quant():
    return O.quant_flat()[0]


# ---------------------------------------------------------------- the reference pin
def test_fixture_cases():
    """The committed file holds the builders' cases, every picture of each, MD5s only."""
    assert _IDS == list(X.CASES)
    for c in EXT:
        assert set(c) == {"name", "refs_md5", "pictures"}
        assert 1 <= len(c["pictures"]) <= 8
        for p in c["pictures"]:
            assert set(p) == {"cfg", "index", "input_md5", "recon_md5", "out_md5"}


@pytest.mark.parametrize("fx", EXT, ids=_IDS)
def test_built_inputs_match_fixture(fx):
    """Builder drift: the inputs built here are the ones the reference decoded."""
    c = X.build(fx["name"])
    assert [p.cfg.as_dict() for p in c.pics] == [p["cfg"] for p in fx["pictures"]]
    assert [p.index for p in c.pics] == [p["index"] for p in fx["pictures"]]
    assert X.digests(c) == dict(inputs=[p["input_md5"] for p in fx["pictures"]], refs=fx["refs_md5"])
    again = X.CASES[fx["name"]](O.lib())              # seeded: a second build is byte-identical
    assert [synth.input_digest(p) for p in again.pics] == X.digests(c)["inputs"] and X.refs_digest(again.refs) == fx["refs_md5"]


@pytest.mark.parametrize("fx", EXT, ids=_IDS)
def test_oracle_matches_reference_md5s(fx):
    """The CPU oracle's reconstruction and output of every picture equal the reference's."""
    c = X.build(fx["name"])
    for i, (p, want) in enumerate(zip(c.pics, fx["pictures"])):
        for stage, key in (("recon", "recon_md5"), ("full", "out_md5")):
            got = O.decode(p, c.refs, stage=stage)
            assert {k: X.md5(got[j]) for j, k in enumerate("YUV")} == want[key], f"picture {i} {stage}"


@pytest.mark.reference
@pytest.mark.skipif(not O.reference_available(), reason="needs the reference sources")
@pytest.mark.parametrize("fx", EXT, ids=_IDS)
def test_live_reference_reproduces_fixture(fx):
    """Every case straight from the compiled reference (milliseconds per picture)."""
    c = X.build(fx["name"])
    for i, (p, want) in enumerate(zip(c.pics, fx["pictures"])):
        rec = O.run_reference(p.cfg, p.index, recon_only=True, inputs=(p, c.refs))
        assert {k: X.md5(rec[j]) for j, k in enumerate("YUV")} == want["recon_md5"], f"picture {i}"
        out = O.run_reference(p.cfg, p.index, inputs=(p, c.refs))
        assert {k: X.md5(out[j]) for j, k in enumerate("YUV")} == want["out_md5"], f"picture {i}"


# ---------------------------------------------------------------- census: R
@pytest.mark.parametrize("name", ["r1_at_bound", "r3_flat_at_bound"])
def test_census_r_at_bound(quant, name):
    """Every coded wave is packed and its largest block is exactly at 32700; the plain-integer
    inverse of such blocks reaches an intermediate of 32700 + 32 and stays inside int16, and the
    residual reaches both (+-32700 + 32) >> 6."""
    c = X.build(name)
    at, big_max, res, lone = 0, 0, set(), set()
    for p in c.pics:
        waves = X.wave_sums(p, quant)
        for (lc, ls, t8, _, _), (lp, _) in zip(waves, X.wave_paths(p, quant)):
            if lc and ls:
                assert not t8 and lp == "packed" and max(ls) == X.PK_RES_MAX, (lp, max(ls))
                at += sum(s == X.PK_RES_MAX for s in ls)
        for _, d in X.luma_blocks(p, quant):
            if sum(abs(v) for r in d for v in r) == X.PK_RES_MAX:
                big, r = X.idct4x4_trace(d)
                assert big <= 32732
                big_max = max(big_max, big)
                res |= {v for row in r for v in row}
                corners = {(i, j): r[i][j] for i in (0, 3) for j in (0, 3)}
                for g, ext in ((1, (X.PK_RES_MAX + 32) >> 6), (-1, (-X.PK_RES_MAX + 32) >> 6)):
                    hit = [k for k, v in corners.items() if v == ext]
                    if len(hit) == 1 and all(abs(v) < abs(ext) - 50 for k, v in corners.items() if k != hit[0]):
                        lone.add((hit[0], g))
    # +- sum |d| on one corner sample alone, for each of the four corners (mass on the odd positions)
    assert lone == {((i, j), g) for i in (0, 3) for j in (0, 3) for g in (1, -1)}, lone
    assert at > 100 and big_max == X.PK_RES_MAX + 32
    assert (X.PK_RES_MAX + 32) >> 6 in res and (-X.PK_RES_MAX + 32) >> 6 in res
    if name.startswith("r3"):
        assert {int(pl[0, 0]) for planes in c.refs for pl in planes} == {0, 255}
        assert {s for p in c.pics for _, _, _, s, _, _ in X.predicted_blocks(p)} >= {0, 1}


@pytest.mark.parametrize("name", ["r2_over", "r3_flat_over"])
def test_census_r_over(quant, name):
    """Every designed wave falls back because of its one designed block: 32701 exactly where the
    scales reach it, sums whose + 32 passes int16, single coefficients on both sides of int16 and at
    40000, residuals past int16 after the shift."""
    c = X.build(name)
    paths = [X.wave_paths(p, quant) for p in c.pics]
    sums = [X.wave_sums(p, quant) for p in c.pics]
    kinds = set()
    for pi, w, kind in c.info["design"]:
        assert paths[pi][w][0] == "fallback", (pi, w, kind)
        ls = sorted(sums[pi][w][1])
        if kind.startswith("sum"):
            assert ls[-1] == int(kind[3:-1]) and ls[-2] <= X.PK_RES_MAX, (kind, ls[-2:])
        kinds.add(kind)
    assert {"sum32701+", "sum32701-", "one<=32767", "one>=32768", "one<=-32768", "one40000", "near2^24"} <= kinds
    assert any(k.startswith("sum3273") or k.startswith("sum3274") for k in kinds)     # + 32 passes 32767
    single = [v for p in c.pics for _, d in X.luma_blocks(p, quant) for v in [[x for r in d for x in r if x]] if len(v) == 1]
    vals = {v[0] for v in single}
    assert any(32767 - 32 < v <= 32767 for v in vals) and any(32768 <= v < 32768 + 64 for v in vals)
    assert any(-32768 - 64 < v <= -32768 for v in vals) and any(40000 - 64 < v <= 40000 for v in vals)
    assert any((v + 32) >> 6 > 32767 for v in vals) and any((v + 32) >> 6 < -32768 for v in vals)
    assert max(abs(v) for v in vals) <= 1 << 24


def test_census_r_chroma(quant):
    """The chroma measure: at the bound every coded wave is packed with its largest measure exactly
    32700, reached by cbpc 1 (DC through the Hadamard) and cbpc 2, with the mass in Cb and in Cr;
    over the bound every designed wave falls back, at 32701 exactly where the scales reach it."""
    c = X.build("r4_chroma_at_bound")
    seen = set()
    for p in c.pics:
        n_at = 0
        for (_, _, _, cc, cs), (_, cp) in zip(X.wave_sums(p, quant), X.wave_paths(p, quant)):
            if cc:
                assert cp == "packed" and max(cs) <= X.PK_RES_MAX
                n_at += sum(s == X.PK_RES_MAX for s in cs)
        assert n_at > 0
        for mi, m in enumerate(p.mbs):
            if int(m["flags"]) & A.MBF_INTRA or not int(m["cbp"]) >> 4:
                continue
            cs = X.wave_sums(X.one_mb(p, mi), quant)[0][4]
            if max(cs) == X.PK_RES_MAX:
                _, cac, _, cdc, _ = X.layout(m)
                o = int(m["coef_off"])
                mass = [int(np.abs(p.levels[o + cdc + 4 * pl:o + cdc + 4 * pl + 4].astype(np.int64)).sum()) for pl in range(2)]
                seen.add((int(m["cbp"]) >> 4, "Cb" if mass[0] > mass[1] else "Cr"))
    assert seen == {(1, "Cb"), (1, "Cr"), (2, "Cb"), (2, "Cr")}, seen
    c = X.build("r4_chroma_over")
    paths = [X.wave_paths(p, quant) for p in c.pics]
    sums = [X.wave_sums(p, quant) for p in c.pics]
    tops = set()
    for pi, w, cbpc in c.info["design"]:
        assert paths[pi][w][1] == "fallback"
        tops.add((cbpc, max(sums[pi][w][4])))
    assert (2, X.PK_RES_MAX + 1) in tops and {k for k, _ in tops} == {1, 2}, tops
    assert all(v <= X.PK_RES_MAX + 16 for _, v in tops), tops


def test_census_r_chroma_cqp(quant):
    """The chroma measure with Cb and Cr dequantised at different QPs (qp_scaled[1] != qp_scaled[2] in
    every MB): each designed MB has one plane at the bound (over the bound in the designed MB of an
    over-bound wave) and the other far below it -- the measure of the MB with its heavy plane's
    levels zeroed stays under 100 -- so a wave's path is decided by the heavy plane's own scales.
    Packed waves at exactly 32700 and fallback waves occur with the heavy plane being Cb and being Cr,
    at 32701 exactly where the plane's scales reach it."""
    c = X.build("r4_chroma_cqp")
    n_at = c.info["at_bound"]
    design = {(pi, w): big for pi, w, _, big in c.info["design"]}
    seen, tops = set(), set()
    assert {tuple(int(v) for v in m["qp_scaled"][1:]) for p in c.pics for m in p.mbs if int(m["mb_type"]) != A.I_PCM} == {(0, 7), (7, 0)}
    for pi, p in enumerate(c.pics):
        assert all(int(m["qp_scaled"][1]) != int(m["qp_scaled"][2]) and [int(v) for v in m["qp_c"]] == [int(v) for v in m["qp_scaled"][1:]]
                   for m in p.mbs)
        paths = X.wave_paths(p, quant)
        heavy = {}
        for mi, m in enumerate(p.mbs):
            if int(m["flags"]) & A.MBF_INTRA or not int(m["cbp"]) >> 4:
                continue
            _, cac, _, cdc, _ = X.layout(m)
            o = int(m["coef_off"])
            span = [[(o + cdc + 4 * pl, 4)] + ([(o + cac + 64 * pl, 64)] if cac is not None else []) for pl in range(2)]
            mass = [sum(int(np.abs(p.levels[a:a + n].astype(np.int64)).sum()) for a, n in span[pl]) for pl in range(2)]
            big = int(mass[1] > mass[0])
            assert max(mass) > 50 * min(mass)
            top = max(X.wave_sums(X.one_mb(p, mi), quant)[0][4])
            light = synth.Picture(p.cfg, p.index, p.mbs[mi:mi + 1], p.levels.copy(), p.mv, p.ref_idx, p.slices, p.pic)
            for a, n in span[big]:
                light.levels[a:a + n] = 0
            assert max(X.wave_sums(light, quant)[0][4]) < 100
            heavy[mi] = (big, top, int(m["qp_scaled"][1 + big]))
        for w, (_, cp) in enumerate(paths):
            mine = [heavy[mi] for mi in range(4 * w, 4 * w + 4) if mi in heavy]
            if not mine:
                continue
            if (pi, w) in design:
                big, top, q = max(mine, key=lambda t: t[1])
                assert cp == "fallback" and big == design[(pi, w)] and top > X.PK_RES_MAX
                assert sum(t > X.PK_RES_MAX for _, t, _ in mine) == 1
                seen.add(("fallback", big))
                tops.add((q, top))
            else:
                assert cp == "packed" and max(t for _, t, _ in mine) <= X.PK_RES_MAX and pi < n_at
                seen |= {("packed", big) for big, t, _ in mine if t == X.PK_RES_MAX}
    assert seen == {(k, pl) for k in ("packed", "fallback") for pl in (0, 1)}, seen
    assert (0, X.PK_RES_MAX + 1) in tops and all(t <= X.PK_RES_MAX + 16 for _, t in tops), tops


@pytest.mark.parametrize("name", ["r5_amplified_intra", "r5_amplified_b", "x_mbaff_p", "x_422_p"])
def test_census_r_amplified(quant, name):
    """amplify(): the gain is the bound's (one more breaks it), the residual saturates samples at 0
    and 255 in every plane, and the MB kinds the case is there for are coded."""
    c = X.build(name)
    assert all(k >= 100 for k in c.info["gains"]), c.info
    for p, k in zip(c.pics, c.info["gains"]):             # one more breaks a bound (or the cap of int16 levels)
        if k < 4000:
            fresh = synth.picture(O.lib(), p.cfg, p.index)
            X.amplify(fresh, k + 1)
            with pytest.raises(AssertionError):
                X.check_bounds(fresh)
    types = set()
    for p in c.pics:
        rec = O.decode(p, c.refs, stage="recon")
        assert all((pl == 0).any() and (pl == 255).any() for pl in rec)
        for m in p.mbs:
            if int(m["cbp"]) or int(m["mb_type"]) == A.I_16x16:
                types.add((int(m["mb_type"]) if int(m["flags"]) & A.MBF_INTRA else "inter", bool(int(m["flags"]) & A.MBF_T8x8),
                           int(m["cbp"]) >> 4))
    if name == "r5_amplified_intra":
        assert {t[0] for t in types} >= {A.I_4x4, A.I_8x8, A.I_16x16} and {t[2] for t in types} == {0, 1, 2}
    else:
        assert ("inter", False, 1) in types and ("inter", False, 2) in types
    if name == "r5_amplified_b":
        assert any(t[0] == "inter" and t[1] for t in types)          # 8x8 blocks feeding the packed construction
    if name == "x_mbaff_p":
        assert any(int(m["flags"]) & A.MBF_FIELD for p in c.pics for m in p.mbs)


# ---------------------------------------------------------------- census: M
def test_census_m_patterns():
    """Over the blocks actually predicted: b1 and h1 reach 10710 and -2550, j1 42 * 10710 and
    -10 * 10710 (the outer products) and the extremes over all 0 / 255 windows, rounded values are
    clipped at both ends, j meets rounding ties ((j1 + 512) a multiple of 1024 with a result the clip
    keeps), and every pattern is read under all 16 phases."""
    cs = {n: X.mc_census(X.build(n)) for n in ("m1_stripes", "m1_outer_random", "m1_flat_checker_b")}
    for n, r in cs.items():
        assert all(len(v) == 16 for v in r["phases"].values()) and len(r["phases"]) >= 4, (n, r["phases"])
    s, o = cs["m1_stripes"], cs["m1_outer_random"]
    assert s["b"] == [-2550, 10710] and s["h"] == [-2550, 10710]
    assert s["bclip"] == {0, 255} and o["jclip"] == {0, 255}
    assert o["j"] == [-2 * 42 * 10 * 255, (42 * 42 + 10 * 10) * 255], o["j"]
    for name, lo, hi in (("outer_max", None, 42 * 10710), ("outer_min", -10 * 10710, None)):
        c = X.build("m1_outer_random")
        slot = ("outer_max", "outer_min", "xnor", "xor", "random").index(name)
        only = X.Case(name, c.pics, [c.refs[slot] if k == slot else tuple(np.full_like(a, 128) for a in c.refs[k])
                                     for k in range(len(c.refs))])
        j = X.mc_census(only)["j"]
        assert (hi is None or j[1] == hi) and (lo is None or j[0] == lo), (name, j)
    assert o["ties"] > 0 and cs["m1_flat_checker_b"]["ties"] > 0
    b = X.build("m1_flat_checker_b")
    assert any(r0 >= 0 and r1 >= 0 for p in b.pics for r0, r1 in zip(p.ref_idx[0].ravel(), p.ref_idx[1].ravel()))


@pytest.mark.parametrize("name", ["m2_borders_p", "m2_borders_b"])
def test_census_m_borders(name):
    """Every border is straddled by the 9x9 luma window by each of 0..8 samples and under each of the
    16 phases (the P case: every corner too, by each amount under each phase), the 3x3 chroma window
    by 0..2, the level-limit vectors are there, and every DPB slot (the generator's plane and two 0 / 255
    patterns) is read."""
    c = X.build(name)
    r = X.mc_census(c)
    assert r["straddle"] == {(b, k) for b in "LRTB" for k in range(9)}
    assert r["straddle_phase"] == {(b, ph) for b in "LRTB" for ph in range(16)}
    assert r["chroma"] == {(b, k) for b in "LRTB" for k in range(3)}
    assert r["mvs"] >= set(X.LIMIT_MVS)
    assert set(r["phases"]) == {0, 1, 2} and all(len(v) == 16 for v in r["phases"].values())
    if name == "m2_borders_p":
        assert c.info["combos"] == 8 * 9 * 16
        assert r["corner"] >= {(cn, k, ph) for cn in ("TL", "TR", "BL", "BR") for k in range(9) for ph in range(16)}
    else:
        assert {cn for cn, _, _ in r["corner"]} == {"TL", "TR", "BL", "BR"}
        assert any((p.ref_idx[0] >= 0).any() and (p.ref_idx[1] >= 0).any() for p in c.pics)


# ---------------------------------------------------------------- census: W
def test_census_w():
    """Every (logWD, weight, offset) of the issue's list is used by a single-list block, for luma and
    chroma; the bi-prediction pairs (127, 127) and (-128, -128) at logWD 0 and (127, -128), (-128, 127)
    at logWD 7; single-list blocks inside B slices; and the value wp_apply4 clips reaches far below 0
    and above 255 (2 * 127 * 255 is past int16 before the shift)."""
    single, pairs, lo, hi = X.wp_census(X.build("w_explicit_p"))
    assert not pairs
    assert single == {(ch, d, w, o) for ch in (False, True) for d in (0, 7) for w, o in X.W_COMBOS}
    assert lo == -128 * 255 - 128 and hi == 127 * 255 + 127
    for name in ("w_explicit_b_flat", "w_explicit_b_random"):
        c = X.build(name)
        single, pairs, lo, hi = X.wp_census(c)
        want = {(ch, 0, 127, 127) for ch in (False, True)} | {(ch, 0, -128, -128) for ch in (False, True)}
        want |= {(ch, 7, 127, -128) for ch in (False, True)} | {(ch, 7, -128, 127) for ch in (False, True)}
        assert want <= pairs, want - pairs
        assert all(-128 <= w0 + w1 <= 127 for _, d, w0, w1 in pairs if d == 7)            # 7.4.3.2
        assert single and lo < -30000 and hi > 30000
        for p in c.pics:
            assert {int(s["luma_log2_wd"]) for s in p.slices} == {0, 7}
            assert all(int(s["luma_log2_wd"]) != int(s["chroma_log2_wd"]) for s in p.slices)


# ---------------------------------------------------------------- census: D
def _line_samples(planes, ln, horizontal):
    n = len(ln["line"]) // 2
    a, e = ln["at"], ln["edge"]
    return [int(v) for v in (planes[ln["plane"]][e - n:e + n, a] if horizontal else planes[ln["plane"]][a, e - n:e + n])]


@pytest.mark.parametrize("name", X.D_LINE_CASES)
def test_census_d_lines(name):
    """Every designed line: the oracle's reconstruction holds the crafted samples, and its output
    holds 8.7.2's filter of them under the edge's designed bS, alpha, beta and tc0 -- so samples change
    exactly where the design says the filter is on, and p1 / q1 / p2 / q2 exactly where ap / aq and the
    strong filter say so."""
    c = X.build(name)
    hz = c.info["horizontal"]
    outs = [(O.decode(p, c.refs, stage="recon"), O.decode(p, c.refs)) for p in c.pics]
    changed = 0
    for ln in c.info["lines"]:
        rec, full = outs[ln["pic"]]
        assert _line_samples(rec, ln, hz) == ln["line"]
        want = X.filter_line(ln["line"], ln["alpha"], ln["beta"], ln["bS"], ln["plane"] > 0, ln["tc0"])
        got = _line_samples(full, ln, hz)
        assert got == want, (ln, got, want)
        if not X.classify(ln["line"], ln["alpha"], ln["beta"], ln["bS"], ln["plane"] > 0, ln["tc0"])["on"]:
            assert got == ln["line"]
        changed += got != ln["line"]
    assert changed > 100


@pytest.mark.parametrize("horizontal", [False, True], ids=["vertical", "horizontal"])
def test_census_d_coverage(horizontal):
    """What the designed lines of one edge direction cover, from their samples and parameters."""
    lines = [dict(ln, case=n) for n in X.D_LINE_CASES if X.build(n).info["horizontal"] == horizontal for ln in X.build(n).info["lines"]]
    cl = [(ln, X.classify(ln["line"], ln["alpha"], ln["beta"], ln["bS"], ln["plane"] > 0, ln["tc0"])) for ln in lines]
    for chroma in (False, True):
        sel = [(ln, c) for ln, c in cl if (ln["plane"] > 0) == chroma and ln["bS"]]
        norm = [(ln, c) for ln, c in sel if ln["bS"] < 4]
        alphas = {ln["alpha"] for ln, _ in norm}
        assert {4, 255} <= alphas and len(alphas) >= 8, alphas        # index 16, mid-range, 51
        assert {ln["bS"] for ln, _ in sel} == {1, 2, 4}
        # alpha: flat sides with a step of alpha - 1 (on), alpha, alpha + 1 (off)
        steps = {(ln["alpha"], c["step"] - ln["alpha"]) for ln, c in norm if c["dp1"] < ln["beta"] and c["dq1"] < ln["beta"]}
        assert {(4, -1), (4, 0), (4, 1), (255, -1), (255, 0)} <= steps
        assert sum({(a, -1), (a, 0), (a, 1)} <= steps for a in alphas) >= 6
        # beta: |p1 - p0| and |q1 - q0| at beta - 1 (on) and beta (off)
        for key in ("dp1", "dq1"):
            other = "dq1" if key == "dp1" else "dp1"
            edge = {(c[key] - ln["beta"], c["on"]) for ln, c in norm if c["step"] < ln["alpha"] and c[other] < ln["beta"] and ln["beta"] > 1}
            assert {(-1, True), (0, False)} <= edge, (key, edge)
        on = [(ln, c) for ln, c in norm if c["on"]]
        assert {c["clip"] for _, c in on} == {-1, 0, 1}               # the delta clipped at + tc and at - tc
        assert {c["clamp"] for _, c in on} >= {0, 255}               # clamp255 acts on p0 + d / q0 - d
        if not chroma:
            # |p2 - p0| and |q2 - q0| at beta - 1 and beta in all four combinations: tc = tc0 + 0 / 1 / 2
            combos = {(c["ap"] - ln["beta"], c["aq"] - ln["beta"]) for ln, c in on}
            assert {(a, b) for a in (-1, 0) for b in (-1, 0)} <= combos, combos
            assert {c["tc"] - ln["tc0"] for ln, c in on} == {0, 1, 2}
            # bS 4: |p0 - q0| at (alpha >> 2) + 1, + 2, + 3, ap / aq true on one side, both, neither
            strong = {(c["step"] - (ln["alpha"] >> 2), c["ap"] < ln["beta"], c["aq"] < ln["beta"])
                      for ln, c in sel if ln["bS"] == 4 and c["on"] and ln["line"][0] != ln["line"][1] and ln["line"][7] != ln["line"][6]}
            assert {(s, a, b) for s in (1, 2, 3) for a in (False, True) for b in (False, True)} <= strong, strong
        else:
            assert any(c["on"] for ln, c in sel if ln["bS"] == 4) and any(not c["on"] for ln, c in sel if ln["bS"] == 4)
    # adjacent 4-line segments of one edge with different bS: 0|1, 1|2, 2|0 (either order)
    pairs, byedge = set(), {}
    for ln in lines:
        if ln["plane"] == 0 and ln["bS"] < 4:
            byedge.setdefault((ln["case"], ln["pic"], ln["edge"]), {})[ln["at"] // 4] = ln["bS"]
    for segs in byedge.values():
        for k in segs:
            if k + 1 in segs and k % 4 != 3:
                pairs.add(frozenset((segs[k], segs[k + 1])))
    assert {frozenset((0, 1)), frozenset((1, 2)), frozenset((2, 0))} <= pairs, pairs


@pytest.mark.parametrize("name", X.D_EVERY_CASES)
def test_census_d_every_edge(name):
    """Inner edges, bS 3, Intra_16x16 at high QP and the 8x8 transform: the oracle's output equals the
    whole loop filter restated from the designed bS of every edge segment (so samples change exactly
    where the design says a filter is on), and the lines of the designed direction, as they stand when
    their edge is filtered, sit on the thresholds for every bS, on MB and on inner edges."""
    c = X.build(name)
    hz = c.info["horizontal"]
    logs, skipped_on = [], 0
    for p, d in zip(c.pics, c.info["design"]):
        rec, full = O.decode(p, c.refs, stage="recon"), O.decode(p, c.refs)
        planes = [a.astype(np.int64) for a in d["want"]]
        assert all(np.array_equal(rec[k], d["want"][k]) for k in range(3))
        X.deblock_restate(planes, 5, 3, d["qp_y"], d["qp_c"], d["bsV"], d["bsH"], d["offa"], d["offb"],
                          log=lambda *a: logs.append(a))
        for k in range(3):
            assert np.array_equal(planes[k], full[k]), (name, k, np.argwhere(planes[k] != full[k])[:3])
        # 8x8-transform MBs: the 4x4 inner edges are not filtered, though a bS 2 line there would be on
        want, out = (d["want"][0].T, full[0].T) if hz else (d["want"][0], full[0])
        kind = [list(r) for r in zip(*d["kind"])] if hz else d["kind"]
        qp = d["qp_y"].T if hz else d["qp_y"]
        for cy, row in enumerate(kind):
            for cx, k in enumerate(row):
                if k != "T":
                    continue
                ia, ib = (min(51, max(0, int(qp[cy][cx]) + o)) for o in (d["offa"], d["offb"]))
                for e in (4, 12):
                    for y in (3, 4, 12):
                        sl = (16 * cy + y, slice(16 * cx + e - 4, 16 * cx + e + 4))
                        assert list(out[sl][3:5]) == list(want[sl][3:5])       # p0, q0: no other edge reaches them
                        skipped_on += X.classify(want[sl], X.ALPHA[ia], X.BETA[ib], 2, False, X.TC0[ia][1])["on"]
    assert skipped_on > 0
    mine = [(pl, inner, bS, al, be, X.classify(line, al, be, bS, pl > 0, tc0), tc0)
            for pl, vertical, inner, mb, bS, al, be, tc0, line in logs if vertical != hz]
    for chroma in (False, True):
        for inner in (False, True):
            sel = [m for m in mine if (m[0] > 0) == chroma and m[1] == inner]
            assert {m[2] for m in sel} == ({1, 2, 3} if inner else {1, 2, 4}), (chroma, inner)
            for bS in {m[2] for m in sel}:
                s = [m for m in sel if m[2] == bS]
                assert any(m[5]["on"] for m in s) and any(not m[5]["on"] for m in s)
                if not inner and bS < 4:
                    continue              # MB edges of bS 1 / 2: the d_bs1 / d_mix cases hold their thresholds
                # |p0 - q0| at alpha - 1 (on) and alpha (off, alpha alone deciding)
                th = {m[5]["step"] - m[3] for m in s if m[3] and m[5]["dp1"] < m[4] and m[5]["dq1"] < m[4]}
                assert {-1, 0} <= th, (chroma, inner, bS, th)
                # |p1 - p0| / |q1 - q0| at beta - 1 and beta
                for key in ("dp1", "dq1"):
                    assert {-1, 0} <= {m[5][key] - m[4] for m in s if m[4] > 1}, (chroma, inner, bS, key)
                assert max(m[3] for m in s if m[5]["on"]) == 255, (chroma, inner, bS)          # indexA 51
                if bS < 4:                # the delta clipped at - tc and at + tc (chroma bS 3: at one end at least)
                    clips = {m[5]["clip"] for m in s if m[5]["on"]}
                    assert clips >= ({-1, 1} if not chroma else {-1}), (chroma, inner, bS, clips)
    luma = [m for m in mine if m[0] == 0]
    # bS 2 with the table's large tc0 (indexA >= 45), inner and MB edges; the strong filter at high alpha
    assert {m[1] for m in luma if m[2] == 2 and m[6] >= 8 and m[5]["on"]} == {False, True}
    strong = {(m[5]["step"] - (m[3] >> 2), m[5]["ap"] < m[4], m[5]["aq"] < m[4]) for m in luma if m[2] == 4 and m[3] >= 200 and m[5]["on"]}
    assert {s for s, _, _ in strong} >= {1, 2, 3} and {(a, b) for _, a, b in strong} >= {(True, True)}, strong
    # adjacent 4-line segments of one INNER edge with different bS
    pairs = set()
    for d in c.info["design"]:
        bs = d["bsH"].T if hz else d["bsV"]
        for bx in range(bs.shape[1]):
            if bx % 4:
                pairs |= {frozenset((int(bs[by, bx]), int(bs[by + 1, bx]))) for by in range(bs.shape[0] - 1) if by % 4 != 3}
    assert {frozenset((0, 2)), frozenset((1, 2))} <= pairs, pairs


# ---------------------------------------------------------------- census: D2
def _d2_walk(name):
    """Per picture of a D2 case: the oracle's reconstruction and output, the restated output, and the
    lines of every edge of bS > 0 as they stand when the restatement filters them:
    (picture, plane, vertical, edge of the MB 0..3, bS, alpha, beta, tc0, line, like luma)."""
    if name not in _d2_walk.done:
        c = X.build(name)
        mw = {0: (16, 16), 1: A.chroma_mb(c.chroma_format), 2: A.chroma_mb(c.chroma_format)}
        pics, lines = [], []
        for pi, p in enumerate(c.pics):
            def probe(pl, vertical, xy, bS, alpha, beta, ia, line, pi=pi):
                if bS:
                    at = xy[0] % mw[pl][0] if vertical else xy[1] % mw[pl][1]
                    e = at // (4 if len(line) == 8 or (c.chroma_format == 2 and not vertical) else 2)
                    lines.append((pi, pl, vertical, e, bS, alpha, beta, X.TC0[ia][bS - 1] if bS < 4 else 0, line, len(line) == 8))
            planes, bs = D2.restate(c, pi, probe=probe)
            pics.append((O.decode(p, c.refs, stage="recon"), O.decode(p, c.refs), planes, bs))
        _d2_walk.done[name] = (pics, lines)
    return _d2_walk.done[name]


_d2_walk.done = {}


@pytest.mark.parametrize("name", X.D2_CASES)
def test_census_d2_restated(name):
    """Every picture of every D2 case: the reconstruction is the crafted planes, and the oracle's
    output equals the whole loop filter restated (strengths from the records by
    extremes_s.strength_restate, the filter by X.deblock_restate with the case's chroma geometry and
    one QP grid per chroma plane), byte for byte; it changes the luma of every picture and each chroma
    plane of most (a plane whose indexA stays below 16 is left as it is, while the other plane of the
    picture is filtered).  A build_d_every case's designed bS of every segment is the restated one."""
    c = X.build(name)
    pics, _ = _d2_walk(name)
    changed = np.zeros((len(pics), 3), bool)
    for pi, (rec, full, planes, (bsV, bsH)) in enumerate(pics):
        d = c.info["design"][pi]
        for k in range(3):
            assert np.array_equal(rec[k], d["want"][k]), (name, pi, k)
            assert np.array_equal(planes[k], full[k]), (name, pi, k, np.argwhere(planes[k] != full[k])[:3])
            changed[pi, k] = not np.array_equal(full[k], rec[k])
        assert changed[pi, 0] and changed[pi, 1:].any(), (name, pi)
        if "bsV" in d:
            assert np.array_equal(bsV, d["bsV"]) and np.array_equal(bsH, d["bsH"]), (name, pi)
        m = c.pics[pi].mbs
        for pl in range(2):             # the records are legal: both chroma QPs follow from qp_y and the picture's offsets
            assert [int(v) for v in m["qp_c"][:, pl]] == [X.qpc_of(q, d["offs"][pl]) for q in m["qp_y"]]
            assert (m["qp_scaled"][:, 1 + pl] == m["qp_c"][:, pl]).all()
        assert (m["qp_y"][m["mb_type"] == A.I_PCM] == 0).all()
    assert (2 * changed.sum(0) > len(pics)).all(), changed
    offs = [d["offs"] for d in c.info["design"]]
    assert all(a != b for a, b in offs) and all(offs[i] != offs[i + 1] for i in range(len(offs) - 1)), offs
    assert all(not np.array_equal(c.info["design"][i]["qp_y"], c.info["design"][i + 1]["qp_y"]) for i in range(len(offs) - 1))


@pytest.mark.parametrize("name", D2.D2_LINE_CASES)
def test_census_d2_lines(name):
    """Every designed line of the build_d cases, as in test_census_d_lines: the reconstruction holds
    it, the output holds 8.7.2's filter of it under the designed bS and the PLANE's own alpha, beta and
    tc0 (4:4:4: the luma filter for Cb and Cr; field pictures: bS 3 on horizontal intra MB edges)."""
    c = X.build(name)
    hz = c.info["horizontal"]
    pics, _ = _d2_walk(name)
    changed = {0: 0, 1: 0, 2: 0}
    for ln in c.info["lines"]:
        rec, full = pics[ln["pic"]][:2]
        chroma = len(ln["line"]) == 4
        assert chroma == (ln["plane"] > 0 and c.chroma_format != 3)
        assert _line_samples(rec, ln, hz) == ln["line"]
        want = X.filter_line(ln["line"], ln["alpha"], ln["beta"], ln["bS"], chroma, ln["tc0"])
        got = _line_samples(full, ln, hz)
        assert got == want, (ln, got, want)
        if not X.classify(ln["line"], ln["alpha"], ln["beta"], ln["bS"], chroma, ln["tc0"])["on"]:
            assert got == ln["line"]
        changed[ln["plane"]] += got != ln["line"]
    assert all(v > 30 for v in changed.values()), changed
    kinds = {(d["kind"], d["structure"]) for d in c.info["design"]}
    if name.startswith("d_field"):
        assert kinds == {(k, s) for k in ("pcm", "bs1") for s in (A.TOP_FIELD, A.BOTTOM_FIELD)}
        assert {ln["bS"] for ln in c.info["lines"]} == ({1, 3} if hz else {1, 4})
    else:
        assert {k for k, _ in kinds} == ({"bs1", "mix", "pcm"} if name.startswith("d_cqp") else {"bs1", "pcm"})


@pytest.mark.parametrize("name", ["d_cqp_v", "d_cqp_h"])
def test_census_d2_cqp_pairs(name):
    """The offset pairs (-12, +12), (+12, -12), an unequal pair of one sign and a pair (0, k); on every MB
    edge Cb's and Cr's lines are different designs; and there are MB edges where one plane has
    indexA < 16 (alpha 0: its samples stay) while the other's lines are filtered, both ways round."""
    c = X.build(name)
    offs = [d["offs"] for d in c.info["design"]]
    assert (-12, 12) in offs and (12, -12) in offs
    assert any(a != b and a * b > 0 for a, b in offs) and any(a == 0 and b != 0 for a, b in offs)
    per = {}
    for ln in c.info["lines"]:
        if ln["plane"]:
            per.setdefault((ln["pic"], ln["edge"], ln["at"] // 8), {1: [], 2: []})[ln["plane"]].append(ln)
    idle = set()
    for key, both in per.items():
        assert [ln["line"] for ln in both[1]] != [ln["line"] for ln in both[2]], key
        for a, b in ((1, 2), (2, 1)):
            if all(ln["alpha"] == 0 for ln in both[a]) and any(
                    ln["bS"] and X.classify(ln["line"], ln["alpha"], ln["beta"], ln["bS"], True, ln["tc0"])["on"] for ln in both[b]):
                idle.add(a)
    assert idle == {1, 2}, idle


def _d2_cells(lines, hz, plane, inner_of=lambda e: e > 0):
    """{(inner, bS): [(alpha, beta, tc0, classification)]} of one plane's lines across the designed direction."""
    cells = {}
    for pi, pl, vertical, e, bS, al, be, tc0, line, luma in lines:
        if pl == plane and vertical != hz:
            cells.setdefault((inner_of(e), bS), []).append((al, be, tc0, X.classify(line, al, be, bS, not luma, tc0), luma))
    return cells


def _d2_thresholds(s, bS, what, sides=True):
    """One cell on its thresholds: a line on and one off; |p0 - q0| at alpha - 1 and at alpha with beta
    not deciding; |p1 - p0| and |q1 - q0| at beta - 1 and at beta; bS < 4: the delta clipped; luma
    filter, bS 4: the step on both sides of (alpha >> 2) + 2 and, with sides, ap / aq true and false on
    either side (build_d_every's cells [c + a, c, c, c + b] have |p2 - p0| == |p1 - p0|, so a line that
    is on has ap and aq true: the sides are the build_d cases')."""
    assert any(m[3]["on"] for m in s) and any(not m[3]["on"] for m in s), what
    th = {m[3]["step"] - m[0] for m in s if m[0] and m[3]["dp1"] < m[1] and m[3]["dq1"] < m[1]}
    assert {-1, 0} <= th, (what, th)
    for key in ("dp1", "dq1"):
        assert {-1, 0} <= {m[3][key] - m[1] for m in s if m[1] > 1}, (what, key)
    if bS < 4:
        assert {m[3]["clip"] for m in s if m[3]["on"]} & {-1, 1}, what
    elif s[0][4]:
        strong = {(m[3]["step"] < (m[0] >> 2) + 2, m[3]["ap"] < m[1], m[3]["aq"] < m[1]) for m in s if m[3]["on"]}
        assert {st for st, _, _ in strong} == {False, True} and (True, True, True) in strong, (what, strong)
        if sides:
            assert {a for _, a, _ in strong} == {False, True} == {b for _, _, b in strong}, (what, strong)


D2_EVERY_BS = {False: {1, 2, 4}, True: {1, 2, 3}}          # MB edges, inner edges


@pytest.mark.parametrize("name", D2.D2_EVERY_CASES)
def test_census_d2_every_edge(name):
    """The build_d_every cases, per PLANE (Cb and Cr sit on different thresholds): across the designed
    direction every bS occurs on MB edges (1, 2, 4) and inner edges (1, 2, 3), and every inner cell
    and every bS 4 cell is on its thresholds (MB edges of bS 1 / 2: the d_cqp / d_bs1 / d_mix cases).
    4:2:2: the chroma edges a 4:2:0 picture does not have -- rows 4 and 12 (bS 2 and 3; bS 1 needs an
    8x8 boundary) -- have lines on and off and a clipped delta per row and bS, and are on the alpha
    and beta thresholds, per plane.  4:4:4: the cells of Cb and Cr
    are the luma's, strong filter included; an 8x8-transform MB's 4x4 edges are idle in all planes."""
    c = X.build(name)
    hz = c.info["horizontal"]
    _, lines = _d2_walk(name)
    n, mb4 = 0, []
    for plane in range(3):
        cells = _d2_cells(lines, hz, plane)
        for inner, want in D2_EVERY_BS.items():
            assert {bS for i, bS in cells if i == inner} == want, (name, plane, inner)
        for (inner, bS), s in cells.items():
            if plane and c.chroma_format != 3 and (inner, bS) == (False, 4):
                # 8 or 16 lines per chroma MB edge and few intra MBs: Cb's and Cr's lines together, as the D
                # census takes them; each plane has a line on and a line off
                assert any(m[3]["on"] for m in s) and any(not m[3]["on"] for m in s), (name, plane)
                mb4 += s
            elif inner or bS == 4:
                _d2_thresholds(s, bS, (name, plane, inner, bS), sides=False)
                n += 1
    if mb4:
        _d2_thresholds(mb4, 4, (name, "Cb + Cr", False, 4))
        n += 1
    if c.chroma_format == 2 and hz:
        for plane in (1, 2):
            odd = []
            for e in (1, 2, 3):
                cells = _d2_cells(lines, hz, plane, inner_of=lambda x: x == e)
                assert {bS for i, bS in cells if i} == ({2, 3} if e & 1 else {1, 2, 3}), (plane, e)
                for bS in (2, 3):
                    s = cells[(True, bS)]
                    assert any(m[3]["on"] for m in s) and any(not m[3]["on"] for m in s), (name, plane, e, bS)
                    assert {m[3]["clip"] for m in s if m[3]["on"]} & {-1, 1}, (name, plane, e, bS)
                    odd += s if e & 1 else []
            # rows 4 and 12 alone (two chroma lines per luma block: few lines each), their bS 2 and 3
            # together (tc0 apart, one filter): on the alpha and beta thresholds
            _d2_thresholds(odd, 2, (name, plane, "rows 4 and 12"))
            n += 1
    if c.chroma_format == 3:
        assert all(luma for *_, luma in lines)
        # 8x8-transform MBs: the 4x4 inner edges are not filtered in any plane, though a bS 2 line there would be on
        skipped_on = [0, 0, 0]
        for d, (rec, full, _, _) in zip(c.info["design"], _d2_walk(name)[0]):
            for my, row in enumerate(d["kind"]):
                for mx, k in enumerate(row):
                    if k != "T":
                        continue
                    for pl in range(3):
                        q = int((d["qp_y"] if pl == 0 else d["qp_c"][pl - 1])[my][mx])
                        ia, ib = (min(51, max(0, q + o)) for o in (d["offa"], d["offb"]))
                        want, out = (rec[pl].T, full[pl].T) if hz else (rec[pl], full[pl])
                        cy, cx = (mx, my) if hz else (my, mx)
                        for e in (4, 12):
                            for y in (3, 4, 12):
                                sl = (16 * cy + y, slice(16 * cx + e - 4, 16 * cx + e + 4))
                                assert list(out[sl][3:5]) == list(want[sl][3:5])       # p0, q0: no other edge reaches them
                                skipped_on[pl] += X.classify(want[sl], X.ALPHA[ia], X.BETA[ib], 2, False, X.TC0[ia][1])["on"]
        assert all(skipped_on), skipped_on
    print(f"D2 census {name}: {n} cells required and hit")


@pytest.mark.parametrize("name", D2.D2_LINE_CASES)
def test_census_d2_line_cells(name):
    """The build_d cases, per plane: MB edges of every bS the case has (d_cqp 1, 2, 4; 4:4:4 1, 4; field
    pictures 1 and 4 on vertical, 1 and 3 on horizontal edges).  Two cells per plane, as bS 1 .. 3
    differ in tc0 alone: the normal filter (its bS together on the alpha and beta thresholds; per bS a
    line on, one off and a clipped delta) and bS 4.  A field picture's bS 3 luma lines reach
    tc0 + 0, + 1 and + 2."""
    c = X.build(name)
    hz = c.info["horizontal"]
    _, lines = _d2_walk(name)
    want = {1, 2, 4} if name.startswith("d_cqp") else {1, 4} if name.startswith("d_444") else {1, 3} if hz else {1, 4}
    n = 0
    for plane in range(3):
        cells = _d2_cells(lines, hz, plane)
        assert {bS for i, bS in cells if not i} == want, (name, plane)
        normal = []
        for bS in want:
            s = cells[(False, bS)]
            if bS == 4:
                _d2_thresholds(s, bS, (name, plane, bS))
                n += 1
            else:
                normal += s
                assert any(m[3]["on"] for m in s) and any(not m[3]["on"] for m in s), (name, plane, bS)
                assert {m[3]["clip"] for m in s if m[3]["on"]} & {-1, 1}, (name, plane, bS)
        _d2_thresholds(normal, 1, (name, plane, "normal"))
        n += 1
        if 3 in want and plane == 0:
            assert {m[3]["tc"] - m[2] for m in cells[(False, 3)] if m[3]["on"]} == {0, 1, 2}
    print(f"D2 census {name}: {n} cells required and hit")


@pytest.mark.parametrize("wrong,name", [(w, n) for w, names in D2.WRONG.items() for n in names])
def test_d2_mutation(wrong, name):
    """A deliberately wrong restatement differs from the oracle's output on some picture of the case,
    so the byte comparison of the GPU with the oracle would notice the same slip in a kernel."""
    c = X.build(name)
    pics, _ = _d2_walk(name)
    for pi in range(len(c.pics)):
        planes, _ = D2.restate(c, pi, wrong=(wrong,))
        if any(not np.array_equal(planes[k], pics[pi][1][k]) for k in range(3)):
            return
    raise AssertionError(f"{name}: the restatement with {wrong} equals the oracle on every picture")


def test_census_x_mbaff_cqp():
    """MBAFF frames with Cb != Cr: frame and field MBs both occur, next to each other in both
    directions; every record is legal under its picture's offsets.
    With the deblocking QPs alone made wrong (extremes_d2.with_qpc: Cb's for Cr and the reverse, or
    QP_C[qp_y] for both) the oracle's reconstruction is the same and its output differs in Cb AND in Cr
    of every picture, and over the case in frame MBs and in field MBs of either plane: a kernel that
    reads the other plane's qp_c, or derives it from qp_y, cannot equal the oracle on this case."""
    c = X.build("x_mbaff_cqp")
    where = set()
    for p, offs in zip(c.pics, c.info["offs"]):
        assert int(p.pic["structure"][0]) == A.MBAFF_FRAME and offs[0] != offs[1]
        W, H = p.cfg.width_mbs, p.cfg.height_mbs
        fld = (p.mbs["flags"].reshape(H, W) & A.MBF_FIELD) != 0
        assert (fld[0::2] == fld[1::2]).all() and (fld[:, 1:] != fld[:, :-1]).any() and (fld[2:] != fld[:-2]).any()
        for pl in range(2):
            assert [int(v) for v in p.mbs["qp_c"][:, pl]] == [X.qpc_of(q, offs[pl]) for q in p.mbs["qp_y"]]
            assert (p.mbs["qp_scaled"][:, 1 + pl] == p.mbs["qp_c"][:, pl]).all()
        rec, full = O.decode(p, c.refs, stage="recon"), O.decode(p, c.refs)
        fld_c = np.repeat(np.repeat(fld[0::2], 16, 0), 8, 1)         # chroma samples of field pairs
        for how in ("swap", "qpy"):
            q = D2.with_qpc(p, how)
            assert all(np.array_equal(a, b) for a, b in zip(O.decode(q, c.refs, stage="recon"), rec))
            other = O.decode(q, c.refs)
            assert np.array_equal(other[0], full[0])
            for k in (1, 2):
                diff = other[k] != full[k]
                assert diff.any(), (p.index, how, k)
                where |= {(how, k, f) for f in (False, True) if diff[fld_c == f].any()}
                print(f"x_mbaff_cqp picture {p.index} {how} plane {k}: {int(diff.sum())} samples differ")
    assert where == {(how, k, f) for how in ("swap", "qpy") for k in (1, 2) for f in (False, True)}, where


# ---------------------------------------------------------------- census: S
S_ROWS = {"s_p_v": {1, 2, 3, 4, 5, 6, 7, 8, 13, 14}, "s_p_h": {1, 2, 3, 4, 5, 6, 7, 8, 13, 14},
          "s_422_v": {1, 2, 3, 4, 5, 6, 7, 8, 14},
          "s_field_v": {1, 2, 3, 4, 5, 6, 7, 8, 13, 14, 9, 10, 11, "11m", 12},
          "s_field_h": {1, 2, 3, 4, 5, 6, 7, 8, 13, 14, 9, 10, 11, "11m", 12},
          "s_b_v": {1, 2, 3, 4, 9, 10, 11, "11m", 12}, "s_b_h": {1, 2, 3, 4, 9, 10, 11, "11m", 12}}


@pytest.mark.parametrize("name", [n for n in X.S_CASES if n != "s_mbaff_v"])
def test_census_s(name):
    """Strength from motion.  From the inputs and the oracle alone: the reconstruction is
    one-dimensional; the plain-Python strength derivation (extremes_s.strength_restate) gives every
    designed segment its designed bS; the loop filter restated from THAT bS equals the oracle's output
    (which pins the oracle's own derivation to a second statement; the edges of the other direction
    are inert only until neighbouring segments of one edge are filtered under different bS, so they
    are restated with everything else rather than asserted idle); every table row has at least 4 live
    segments (bS 1 would change one of its lines as the walk meets them) and at most 1 designed
    segment in 20 is dead; both polarities of every signed difference occur; the B cases hold every
    single-list row under both dispatches of inter4_one_list."""
    import extremes_s as S
    c = X.build(name)
    hz = c.info["horizontal"]
    rows_live, rows_all, dead, total = {}, {}, 0, 0
    signs, row8, dispatch = set(), set(), {}
    for p, d in zip(c.pics, c.info["design"]):
        W, H = p.cfg.width_mbs, p.cfg.height_mbs
        rec, full = O.decode(p, c.refs, stage="recon"), O.decode(p, c.refs)
        for k in range(3):
            a = rec[k].T if hz else rec[k]
            assert (a == a[0]).all(), (name, k)
        bsV, bsH = S.strength_restate(p)
        mine = bsH.T if hz else bsV
        assert set(np.unique(bsV)) | set(np.unique(bsH)) <= {0, 1}
        for s in d["segs"]:
            assert int(mine[s["r"], s["c"]]) == s["bs"], (name, p.index, s)
        live = {}

        def probe(pl, vertical, xy, bS, alpha, beta, ia, line):
            if vertical != hz and pl == 0:
                key = (xy[1] // 4, xy[0] // 4) if hz else (xy[0] // 4, xy[1] // 4)
                live[key] = live.get(key, False) or X.filter_line(line, alpha, beta, 1, False, X.TC0[ia][0]) != line
        planes = [a.astype(np.int64) for a in rec]
        qp_y = np.full((H, W), d["qp"])
        X.deblock_restate(planes, W, H, qp_y, np.full((H, W), X.QP_C[d["qp"]]), bsV, bsH, 0, 0, probe=probe)
        for k in range(1 if c.chroma_format == 2 else 3):       # (the restatement's chroma is 4:2:0)
            assert np.array_equal(planes[k], full[k]), (name, p.index, k, np.argwhere(planes[k] != full[k])[:3])
        assert not np.array_equal(full[0], rec[0])
        one = S.one_list_waves(p)
        for s in d["segs"]:
            lv = live[(s["c"], s["r"])]
            total, dead = total + 1, dead + (not lv)
            rows_all[s["row"]] = rows_all.get(s["row"], 0) + 1
            rows_live[s["row"]] = rows_live.get(s["row"], 0) + lv
            if lv:
                signs.add((s["row"], s["sx"], s["sy"], s["bs"]))
                if s["row"] == 8:
                    row8.add((s["same_idx"], s["same_pic"], s["bs"]))
                x4, y4 = (s["r"], s["c"]) if hz else (s["c"], s["r"])
                if s["single"] and s["row"] in (1, 2, 3, 4) and int(p.ref_idx[1, y4, x4]) < 0:
                    dispatch.setdefault(s["row"], set()).add(one[((y4 // 4) * W + x4 // 4) // 4])
    assert set(rows_all) == S_ROWS[name], set(rows_all) ^ S_ROWS[name]
    assert all(rows_live[r] >= 4 for r in rows_all), rows_live
    assert dead * 20 <= total, (dead, total, {r: rows_all[r] - rows_live[r] for r in rows_all})
    if name.startswith("s_field"):
        assert c.info["lim"] == 2 and {int(p.pic["structure"][0]) for p in c.pics} == {A.TOP_FIELD, A.BOTTOM_FIELD}
        # |dmvy| 2 and 3 are far in a field; the other parity of one slot is another picture
        assert {b for r, _, sy, b in signs if r == 3 and sy} == {0, 1} and rows_live[7] >= 4
    for sg in (1, -1):
        assert {(2, sg, 0, 0), (2, sg, 0, 1), (3, 0, sg, 0), (3, 0, sg, 1)} <= signs, signs      # +-(limit - 1) -> 0, +-limit -> 1
        for sh in (1, -1):
            assert {(4, sg, sh, 0), (4, sg, sh, 1)} <= signs
    if name.startswith("s_b"):
        assert all(dispatch.get(r) == {False, True} for r in (1, 2, 3, 4)), dispatch
    if name.startswith(("s_b", "s_field")):
        assert {w for p in c.pics for w in p.slices["wp_mode"]} == {0, 1}
        for r in (9, 10, 11, 12):
            assert {b for rr, _, _, b in signs if rr == r} == {0, 1}, r
    if not name.startswith("s_b"):
        # row 8: one ref_idx number naming two pictures -> 1; two numbers naming one picture -> by vector
        assert {(True, False, 1), (False, True, 0), (False, True, 1)} <= row8, row8
        assert {b for rr, _, _, b in signs if rr == 5} == {0, 1} and {b for rr, _, _, b in signs if rr == 6} == {0, 1}


def test_census_s_mbaff():
    """MBAFF, vertical edges.  Every block column is uniform along y (asserted on the inputs: MB kind,
    ref_idx, vectors), so every horizontal edge compares identical motion of one kind and is idle, and
    the oracle's output is one-dimensional like its reconstruction (asserted).  One row, its vertical
    edges filtered left to right under the restated bS (extremes_s.strength_restate_mbaff_v), is
    therefore the whole loop filter: it equals every row of the oracle's output.  Rows 1-7 are live
    between two frame MBs and between two field MBs, row 15 between a frame and a field MB."""
    import extremes_s as S
    c = X.build("s_mbaff_v")
    live_rows, dead, total = {}, 0, 0
    for p, d in zip(c.pics, c.info["design"]):
        assert int(p.pic["structure"][0]) == A.MBAFF_FRAME
        W, H = p.cfg.width_mbs, p.cfg.height_mbs
        for a in (p.ref_idx, p.mv, p.mbs["flags"].reshape(H, W), p.mbs["slice"].reshape(H, W)):
            assert (a == a[..., :1, :]).all()                   # uniform along y
        assert {int(f) & A.MBF_FIELD for f in p.mbs["flags"]} == {0, A.MBF_FIELD}
        rec, full = O.decode(p, c.refs, stage="recon"), O.decode(p, c.refs)
        assert all((a == a[0]).all() for a in rec) and all((a == a[0]).all() for a in full)
        bsV = S.strength_restate_mbaff_v(p)
        assert (bsV == bsV[0]).all()
        for s in d["segs"]:
            assert int(bsV[0, s["c"]]) == s["bs"], (p.index, s)
        qp, qpc = d["qp"], X.QP_C[d["qp"]]
        rows = [[int(v) for v in rec[k][0]] for k in range(3)]
        live = {}
        for x4 in range(1, 4 * W):
            bS = int(bsV[0, x4])
            for pl in range(3):
                if pl and x4 & 1:
                    continue
                n, x, q = (4, 4 * x4, qp) if pl == 0 else (2, 2 * x4, qpc)
                line = rows[pl][x - n:x + n]
                if pl == 0:
                    live[x4] = X.filter_line(line, X.ALPHA[q], X.BETA[q], 1, False, X.TC0[q][0]) != line
                if bS:
                    rows[pl][x - n:x + n] = X.filter_line(line, X.ALPHA[q], X.BETA[q], bS, pl > 0, X.TC0[q][bS - 1])
        for k in range(3):
            assert (full[k] == np.array(rows[k], np.uint8)).all(), (p.index, k)
        assert rows[0] != [int(v) for v in rec[0][0]]
        for s in d["segs"]:
            total, dead = total + 4 * H, dead + (0 if live[s["c"]] else 4 * H)
            if live[s["c"]]:
                key = (s["row"], s["field"])
                live_rows.setdefault(key, set()).add((s["sx"], s["sy"], s["bs"]))
    assert dead * 20 <= total, (dead, total)
    for row in range(1, 8):
        for fld in (False, True):
            if (row, fld) == (7, False):
                assert {b for _, _, b in live_rows[(row, fld)]} == {1}      # another frame
                continue
            want = {1: {0}, 7: {1}}.get(row, {0, 1})
            assert {b for _, _, b in live_rows[(row, fld)]} == want, (row, fld)
    assert {b for _, _, b in live_rows[(15, False)]} == {1} and {b for _, _, b in live_rows[(15, True)]} == {1}
    for fld in (False, True):
        for sg in (1, -1):
            assert {(sg, 0, 0), (sg, 0, 1)} <= live_rows[(2, fld)] and {(0, sg, 0), (0, sg, 1)} <= live_rows[(3, fld)]
            assert any(sx == sg and b == 0 for sx, _, b in live_rows[(4, fld)]) and any(sy == sg and b == 1 for _, sy, b in live_rows[(4, fld)])


# ---------------------------------------------------------------- census: I
def _i_tags(name):
    return {(s["pic"], s["mb"]): s for s in X.build(name).info["sites"]}


@pytest.mark.parametrize("name", I.I_RESTATED)
def test_census_i_restated(name):
    """Intra prediction restated (extremes_i.intra_restate: 8.3 in Python integers, availability by
    6.4.12 from the records alone) equals the oracle's reconstruction of every picture byte for byte;
    the output is the reconstruction (deblock_idc 1 everywhere); every intra MB is without residual
    unless it is in the chain; every site stands alone at dependency level 1; and the availability
    bits the restatement derived for each block are the ones the block geometry (avail4 / avail8) gives for the mask
    its builder designed."""
    c = X.build(name)
    entries, equal = I.census(name)
    assert all(equal), (name, equal)
    tags = _i_tags(name)
    for pi, p in enumerate(c.pics):
        assert all(int(s["deblock_idc"]) == 1 for s in p.slices)
        assert all(np.array_equal(a, b) for a, b in zip(O.decode(p, c.refs), O.decode(p, c.refs, stage="recon")))
        lv = I.levels_of(p)
        W = p.cfg.width_mbs
        for a, m in enumerate(p.mbs):
            if int(m["flags"]) & A.MBF_INTRA and int(m["mb_type"]) != A.I_PCM:
                s = tags[(pi, (a % W, a // W))]
                assert s["tag"] == "chain" or (int(m["cbp"]) == 0 and int(m["cbp_blks"]) == 0 and lv[a // W, a % W] == 1)
    for e in entries:
        mask = tags[(e["pic"], e["mb"])]["mask"]
        if e["kind"] in ("i4", "i8"):
            want = (I.avail4 if e["kind"] == "i4" else I.avail8)(e["blk"], mask)
            got = e["bits"]
            assert (got[0], got[1], got[3]) == (want[0], want[1], want[3]) and (not got[1] or got[2] == want[2]), (name, e["mb"], e["blk"])
        else:
            assert e["bits"] == (mask[0], mask[1], mask[3])


def _i_random_entries(names):
    """The logged blocks of the sites whose neighbours are seeded random bytes."""
    out = []
    for n in names:
        tags = _i_tags(n)
        out += [e for e in I.census(n)[0] if tags[(e["pic"], e["mb"])]["tag"] in ("mask", "border", "slice", "chain")]
    return out


def _i_cells(entries, chroma_blocks):
    """Per kind (required cells, cells hit): a cell is hit when, among its blocks with random
    neighbours, one changes under EVERY other legal mode and, for each availability bit the mode
    reads, one changes when that bit is flipped (the poison, or the other sum, comes into play).  A
    flip of a bit the mode does not read must change nothing, anywhere."""
    req = I.required_cells(chroma_blocks)
    modes_ok = {k: set() for k in req}
    flips_ok = {k: {} for k in req}
    need = {k: {} for k in req}
    for e in entries:
        kind, mode, bits = e["kind"], e["mode"], e["bits"]
        group = kind if kind in ("i4", "i8", "i16") else "c"
        cell = I.cell_of(e)
        assert cell in req[group], (group, cell)
        rd = I.reads(kind, mode, bits)
        if not (group == "c" and mode == 0):
            for i, changed in e["flips"].items():
                assert i in rd or not changed, (kind, mode, bits, i)
        need[group].setdefault(cell, set()).update(i for i in rd)
        if e["others"]:
            modes_ok[group].add(cell)
        for i in rd:
            if e["flips"].get(i):
                flips_ok[group].setdefault(cell, set()).add(i)
        if group == "c" and mode == 0:
            for blk, _, _ in e["blocks"]:
                xO, yO = (blk & 1) * 4, (blk >> 1) * 4
                dcell = (kind, blk, bits[0], bits[1])
                use = I.chroma_dc_uses(xO, yO, bits[0], bits[1])
                if e["blk_others"][blk]:
                    modes_ok["cdc"].add(dcell)
                for i in (0, 1):
                    nb = (bits[0] ^ (i == 0), bits[1] ^ (i == 1))
                    eff = I.chroma_dc_uses(xO, yO, *nb) != use
                    if i in e["blk_flips"]:
                        assert eff or not e["blk_flips"][i][blk], (dcell, i)
                        if eff:
                            need["cdc"].setdefault(dcell, set()).add(i)
                            if e["blk_flips"][i][blk]:
                                flips_ok["cdc"].setdefault(dcell, set()).add(i)
    hit = {k: {c for c in req[k] if c in modes_ok[k] and flips_ok[k].get(c, set()) >= need[k].get(c, set())} for k in req}
    return req, hit


def test_census_i_cells():
    """Every (mode, block, availability) cell the legality rules and the block geometry allow occurs
    in the plain 4:2:0 cases with random neighbours, and every such cell passes the mutation check."""
    req, hit = _i_cells(_i_random_entries(I.I_PLAIN), 4)
    for k in req:
        print(f"I census {k}: required {len(req[k])} hit {len(hit[k])}")
    for k in req:
        assert hit[k] == req[k], (k, sorted(req[k] - hit[k])[:8])
    assert {k: len(v) for k, v in req.items()} == I.CELL_COUNTS


def test_census_i_422():
    """The 4:2:2 chroma predictor: every (mode, availability) cell of both planes and every DC cell of
    the eight 4x4 chroma blocks, mutation-checked; luma Intra_16x16 cells with them."""
    req, hit = _i_cells(_i_random_entries(["i_422"]), 8)
    for k in ("i16", "c", "cdc"):
        print(f"I census 4:2:2 {k}: required {len(req[k])} hit {len(hit[k])}")
        assert hit[k] == req[k], (k, sorted(req[k] - hit[k])[:8])
    assert len(req["cdc"]) == 2 * 8 * 4


@pytest.mark.parametrize("name", ["i_top", "i_bottom"])
def test_census_i_fields(name):
    """A field picture's sites: all three MB kinds, all four chroma modes, all 16 masks."""
    c = X.build(name)
    want = A.TOP_FIELD if name == "i_top" else A.BOTTOM_FIELD
    assert [int(p.pic["structure"][0]) for p in c.pics] == [want]
    entries = I.census(name)[0]
    assert {e["kind"] for e in entries} == {"i4", "i8", "i16", "cb", "cr"}
    assert {e["mode"] for e in entries if e["kind"] == "cb"} == {0, 1, 2, 3}
    assert {e["mode"] for e in entries if e["kind"] == "i4"} == set(range(9)) == {e["mode"] for e in entries if e["kind"] == "i8"}
    assert {s["mask"] for s in c.info["sites"]} == set(I.MASKS)


def test_census_i_values():
    """Every (MB kind, mode) over neighbours that are all 0, all 255, 0 / 255 alternating in both
    phases and ramps in both directions: the four neighbour MBs hold exactly that pattern."""
    seen = set()
    for n in ("i_4x4", "i_8x8", "i_16x16", "i_422"):
        c = X.build(n)
        tags = _i_tags(n)
        ch = A.chroma_mb(c.chroma_format)[1]
        for e in I.census(n)[0]:
            s = tags[(e["pic"], e["mb"])]
            if s["tag"] != "values" or e["blk"] != 0:
                continue
            pat = s["pat"]["A"]
            assert set(s["pat"].values()) == {pat} and s["mask"] == (1, 1, 1, 1)
            mx, my = e["mb"]
            for nx, ny in ((mx - 1, my), (mx, my - 1), (mx + 1, my - 1), (mx - 1, my - 1)):
                for k, (w, h) in enumerate(((16, 16), (8, ch), (8, ch))):
                    assert np.array_equal(c.refs[e["pic"]][k][h * ny:h * ny + h, w * nx:w * nx + w], I.pattern_mb(pat, w, h, None))
            seen.add((("c422" if e["kind"] in ("cb", "cr") else e["kind"]) if n == "i_422" else e["kind"], e["mode"], pat))
    want = {(k, m, pat) for pat in I.PATTERNS for k, nm in (("i4", 9), ("i8", 9), ("i16", 4), ("cb", 4), ("cr", 4), ("c422", 4))
            for m in range(nm)}
    assert want <= seen, sorted(want - seen)[:8]


def test_census_i_dc_rounding():
    """For every DC form and each of its two shifts: a neighbour sum whose remainder mod 2^shift is
    2^(shift - 1) - 1 (the last that rounds down) and one at 2^(shift - 1) (the first that rounds up)."""
    got = {}
    for n in I.I_RESTATED:
        for e in I.census(n)[0]:
            key = e["kind"] + ("/422" if n == "i_422" and e["kind"] in ("cb", "cr") else "")
            if "dc" in e:
                got.setdefault(key, set()).add(e["dc"])
            for _, sh, rem in e.get("blocks", ()):
                if rem is not None:
                    got.setdefault(key, set()).add((sh, rem))
    for kind, shifts in list(I.DC_SHIFTS.items()) + [("cb/422", (2, 3)), ("cr/422", (2, 3))]:
        for sh in shifts:
            assert {(sh, (1 << (sh - 1)) - 1), (sh, 1 << (sh - 1))} <= got[kind], (kind, sh)


def test_census_i_plane():
    """The plane predictors at their extremes, from the logged unclipped values: Intra_16x16 Hs and
    Vs at +-9180 = 255 (1 + .. + 8); chroma +-2550 = 255 (1 + .. + 4) in 4:2:0 and, vertically, +-9180 in
    4:2:2 (8.3.4.4 with yCF = 4: eight terms); per kind an MB whose samples clip at 0 AND at 255, and
    one without any clipping."""
    for n, kinds in (("i_16x16", (("i16", 9180, 9180), ("cb", 2550, 2550), ("cr", 2550, 2550))),
                     ("i_422", (("i16", 9180, 9180), ("cb", 2550, 9180), ("cr", 2550, 9180)))):
        for kind, hmax, vmax in kinds:
            pl = [e["plane"] for e in I.census(n)[0] if e["kind"] == kind and "plane" in e]
            assert {hmax, -hmax} <= {h for h, _, _, _ in pl} and {vmax, -vmax} <= {v for _, v, _, _ in pl}, (n, kind)
            assert max(abs(h) for h, _, _, _ in pl) == hmax and max(abs(v) for _, v, _, _ in pl) == vmax
            assert any(lo < 0 and hi > 255 for _, _, lo, hi in pl), (n, kind)
            assert any(lo >= 0 and hi <= 255 for _, _, lo, hi in pl), (n, kind)


def test_census_i_edges():
    """Unavailability by the picture border and by a slice boundary, not by CIP: the border picture is
    an I picture of intra MBs alone with sites on all four corners and edges; in the slice picture
    every MB is intra and every neighbour a site misses lies in another slice."""
    c = X.build("i_edges")
    W, H = c.pics[0].cfg.width_mbs, c.pics[0].cfg.height_mbs
    border = {s["mb"]: s["mask"] for s in c.info["sites"] if s["pic"] == 0}
    assert int(c.pics[0].slices[0]["slice_type"]) == A.SLICE_I and not int(c.pics[0].pic["constrained_intra_pred"][0])
    assert all(int(m["flags"]) & A.MBF_INTRA for p in c.pics for m in p.mbs)
    for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (4, 0), (4, H - 1), (0, 4), (W - 1, 4)):
        assert border[(x, y)] == (int(x > 0), int(y > 0), int(y > 0 and x < W - 1), int(x > 0 and y > 0))
    assert set(border.values()) == {(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 1, 0), (1, 1, 0, 1), (1, 1, 1, 1)}
    sl = {s["mb"]: s["mask"] for s in c.info["sites"] if s["pic"] == 1}
    p = c.pics[1]
    assert len(set(int(s) for s in p.mbs["slice"])) == 4 and int(p.pic["constrained_intra_pred"][0]) == 1
    assert sl[(7, 3)] == (0, 0, 0, 0) and sl[(9, 3)] == (1, 0, 0, 0) and sl[(4, 3)] == (1, 1, 1, 1)
    assert sl[(3, 10)] == (1, 0, 0, 0) and sl[(6, 10)] == (1, 0, 1, 0) and sl[(7, 14)] == (1, 1, 1, 0) and sl[(10, 14)] == (1, 1, 1, 1)
    assert {e["kind"] for e in I.census("i_edges")[0] if e["pic"] == 1} == {"i4", "i8", "i16", "cb", "cr"}


def test_census_i_chain():
    """The chain: in every chain row the dependency levels run 1 .. 7 left to right (so levels above
    the three list levels exist), the MBs at even levels carry a residual, every list level holds
    pairable MBs and others, and the residuals are small."""
    c = X.build("i_chain")
    assert len(c.pics) == 2
    for p in c.pics:
        lv = I.levels_of(p)
        W = p.cfg.width_mbs
        for y in range(1, p.cfg.height_mbs, 2):
            assert list(lv[y, 1:1 + I.CHAIN_LEN]) == list(range(1, I.CHAIN_LEN + 1))
            coded = [int(p.mbs[y * W + x]["cbp"]) != 0 for x in range(1, 1 + I.CHAIN_LEN)]
            assert coded == [i % 2 == 1 for i in range(I.CHAIN_LEN)] and sum(coded) * 2 >= I.CHAIN_LEN - 1
        assert I.CHAIN_LEN >= 6 and lv.max() == I.CHAIN_LEN
        for level in (1, 2, 3):
            kinds = [int(p.mbs[a]["mb_type"]) for a in range(len(p.mbs)) if lv.ravel()[a] == level]
            assert kinds.count(A.I_4x4) >= 2 and (level == 2 or len(kinds) > kinds.count(A.I_4x4))
        assert int(np.abs(p.levels[[int(m["coef_off"]) for m in p.mbs if int(m["cbp"])]].astype(np.int64)).max()) <= 8


def test_census_i_pairs():
    """The pair list of level 1 (I_4x4, not lossless): over all pictures of a plain case and over all
    but the last its count has different parities, so one of the two batches leaves a single MB over."""
    for n in I.I_PLAIN:
        c = X.build(n)
        counts = [I.pairable_level1(p) for p in c.pics]
        print(n, "level-1 pairable MBs per picture", counts)
        assert len(c.pics) >= 2 and counts[-1] % 2 == 1 and sum(counts) > 2, (n, counts)


def test_census_i_mbaff():
    """The weaker census of the generated MBAFF case (no restatement: it is pinned to the reference
    alone): every (kind, mode) occurs in a frame MB and in a field MB, every I_4x4 (blkIdx, mode) and
    I_8x8 (blk, mode) occurs; no intra MB has a residual; the I_PCM MBs hold the value patterns."""
    c = X.build("i_mbaff")
    assert c.info == dict(seed=I.MBAFF_SEED, size=(I.MBAFF_W, I.MBAFF_H))
    kinds, c4, c8 = I.mbaff_census(c)
    print(f"I census MBAFF: (kind, mode, frame / field) {len(kinds)} of 52, I_4x4 (blkIdx, mode) {len(c4)} of 144, "
          f"I_8x8 (blk, mode) {len(c8)} of 36")
    want = {(k, m, f) for k, n in (("i4", 9), ("i8", 9), ("i16", 4), ("c", 4)) for m in range(n) for f in (False, True)}
    assert kinds == want, sorted(want - kinds)
    assert c4 == {(b, m) for b in range(16) for m in range(9)} and c8 == {(b, m) for b in range(4) for m in range(9)}
    flat = set()
    for p in c.pics:
        assert int(p.pic["structure"][0]) == A.MBAFF_FRAME and int(p.pic["constrained_intra_pred"][0]) == 1
        for m in p.mbs:
            if int(m["mb_type"]) == A.I_PCM:
                raw = p.levels[int(m["coef_off"]):int(m["coef_off"]) + 128].view(np.uint8)
                flat |= {int(raw[0])} if (raw == raw[0]).all() else set()
            elif int(m["flags"]) & A.MBF_INTRA:
                assert int(m["cbp"]) == 0 and int(m["cbp_blks"]) == 0
    assert flat == {0, 255}


# ---------------------------------------------------------------- census: d_mbaff
MBAFF_CLASS_BS = {      # the bS an edge class can take in these pictures (intra, coded, frame MB against field MB, else none)
    "V1": {4, 2}, "V2": {4, 2}, "V3t": {4, 2, 1}, "V3b": {4, 2, 1}, "V4t": {4, 2, 1}, "V4b": {4, 2, 1},
    "H1": {4, 2}, "H3": {4, 2}, "H2a": {3, 2, 1}, "H2b": {3, 2, 1}, "H4": {3, 2}, "H6": {3, 2},
    "H5": {3, 2, 1}, "H7": {3, 2, 1}, "Inner-v": {3, 2}, "Inner-h-frame": {3, 2}, "Inner-h-field": {3, 2},
}


def _mbaff_walk():
    """Per picture of d_mbaff the oracle's output and the restated one, and the restatement's log with the
    picture index in front: (pi, plane, vertical, class, p MB address, bS, alpha, beta, tc0, line, coords)."""
    if not _mbaff_walk.done:
        c = X.build("d_mbaff")
        for pi, p in enumerate(c.pics):
            log = []
            planes = D2.restate_mbaff(c, pi, log=lambda *a: log.append(a))
            _mbaff_walk.done.append((O.decode(p, c.refs), planes, [(pi,) + a for a in log]))
    return _mbaff_walk.done


_mbaff_walk.done = []


def test_census_d_mbaff_restated():
    """Every picture: MBAFF frame of 4 x 6 MBs, deblock_idc 0 (the last picture's second slice 2), the
    reconstruction is the crafted planes, and the oracle's output equals deblock_restate_mbaff byte for
    byte.  The pair kinds hold all four (current, left) and (current, upper) combinations; all four MB
    kinds occur in frame and in field MBs; the two MBs of every pair differ in qp_y (by 7 or more, so
    that their averages with a third MB give different alpha), in both qp_c, and in which of their
    edge blocks are coded;
    the records are legal."""
    c = X.build("d_mbaff")
    kinds = set()
    for pi, (p, d, (full, planes, _)) in enumerate(zip(c.pics, c.info["design"], _mbaff_walk())):
        W, H = p.cfg.width_mbs, p.cfg.height_mbs
        assert (W, H) == (4, 6) and int(p.pic["structure"][0]) == A.MBAFF_FRAME and int(p.pic["constrained_intra_pred"][0]) == 1
        assert [int(s["deblock_idc"]) for s in p.slices] == ([0, 2] if pi == len(c.pics) - 1 else [0])
        rec = O.decode(p, c.refs, stage="recon")
        for k in range(3):
            assert np.array_equal(rec[k], d["want"][k]), (pi, k)
            assert np.array_equal(planes[k], full[k]), (pi, k, np.argwhere(planes[k] != full[k])[:4])
            assert not np.array_equal(full[k], rec[k])
        f = d["fld"]
        assert {(bool(f[r, x]), bool(f[r, x - 1])) for r in range(3) for x in range(1, W)} == {(a, b) for a in (False, True) for b in (False, True)}
        assert {(bool(f[r, x]), bool(f[r - 1, x])) for r in range(1, 3) for x in range(W)} == {(a, b) for a in (False, True) for b in (False, True)}
        m = p.mbs.reshape(H, W)
        assert ((m["flags"] & A.MBF_FIELD != 0) == np.repeat(f, 2, 0)).all()
        for pl in range(2):
            assert [int(v) for v in p.mbs["qp_c"][:, pl]] == [X.qpc_of(q, d["offs"][pl]) for q in p.mbs["qp_y"]]
            assert (p.mbs["qp_scaled"][:, 1 + pl] == p.mbs["qp_c"][:, pl]).all()
        top, bot = m[0::2], m[1::2]
        assert (np.abs(top["qp_y"].astype(int) - bot["qp_y"]) >= 7).all() and (top["qp_c"] != bot["qp_c"]).all()
        assert ((top["cbp_blks"] & 0xF99F) != (bot["cbp_blks"] & 0xF99F)).all()          # the blocks along the MB's four edges
        kinds |= {(str(k), bool(f[y // 2, x])) for y in range(H) for x in range(W) for k in d["kind"][y, x]}
    assert kinds == {(k, fl) for k in "CPDI" for fl in (False, True)}, kinds


def _mbaff_cells():
    cells = {}
    for _, _, log in _mbaff_walk():
        for pi, pl, vertical, cls, pa, bS, al, be, tc0, line, coords in log:
            if cls == "Inner":
                cls = "Inner-v" if vertical else "Inner-h-field" if coords[1][0] - coords[0][0] == 2 else "Inner-h-frame"
            cells.setdefault((cls, pl, bS), []).append((al, be, tc0, X.classify(line, al, be, bS, pl > 0, tc0)))
    return cells


# what the pictures cannot reach, with the reason: (cell, item) -> reason.  Luma alone: an I_PCM MB's chroma QP
# is QP_C[offset], and its inner chroma edges are live and required wherever that plus the FilterOffset reaches 16.
_INSIDE_INTRA_LUMA = ("luma bS 3 lies inside an intra MB, and the two intra kinds whose samples are known by construction "
                      "are I_PCM (qp_y 0: luma indexA <= 12, alpha 0, every line off) and the flat Intra_16x16 DC MB (no "
                      "step: every line on, nothing to clip)")
MBAFF_UNREACHABLE = {((cls, 0, 3), item): _INSIDE_INTRA_LUMA for cls in ("Inner-v", "Inner-h-frame", "Inner-h-field")
                     for item in ("alpha-1", "alpha", "beta-1", "beta", "clip")}


def test_census_d_mbaff_cells():
    """Every (edge class, plane, bS) the rules allow, from the lines as they stand when the restatement
    filters them: a line on and one off; |p0 - q0| at alpha - 1 and at alpha with beta not deciding;
    |p1 - p0| or |q1 - q0| at beta - 1 and at beta; bS < 4: the delta clipped at one end at least; luma
    bS 4: the step on both sides of (alpha >> 2) + 2 with ap / aq true and false.  No class takes a bS
    outside its set."""
    cells = _mbaff_cells()
    req = {(cls, pl, bS) for cls, bss in MBAFF_CLASS_BS.items() for pl in range(3) for bS in bss}
    assert set(cells) <= req, sorted(set(cells) - req)
    missing = []
    for cell in sorted(req):
        s = cells.get(cell, [])
        bS, chroma = cell[2], cell[1] > 0
        on = [m for m in s if m[3]["on"]]
        need = {"on": bool(on), "off": len(on) < len(s)}
        th = {m[3]["step"] - m[0] for m in s if m[0] and m[3]["dp1"] < m[1] and m[3]["dq1"] < m[1]}
        need["alpha-1"], need["alpha"] = -1 in th, 0 in th
        bt = {m[3][k] - m[1] for m in s if m[1] > 1 for k in ("dp1", "dq1")}
        need["beta-1"], need["beta"] = -1 in bt, 0 in bt
        if bS < 4:
            need["clip"] = bool({m[3]["clip"] for m in on} & {-1, 1})
        elif not chroma:
            st = {(m[3]["step"] < (m[0] >> 2) + 2, m[3]["ap"] < m[1], m[3]["aq"] < m[1]) for m in on}
            need["strong"] = {a for a, _, _ in st} == {False, True} and {b for _, b, _ in st} == {False, True} == {b for _, _, b in st}
        bad = sorted(k for k, v in need.items() if not v and (cell, k) not in MBAFF_UNREACHABLE)
        if bad:
            missing.append((cell, len(s), bad))
    named = {cell for cell, _ in MBAFF_UNREACHABLE}
    print(f"d_mbaff census: {len(req)} cells required, {len(req) - len(missing)} hit, of them {len(named)} (luma inner bS 3) on / off only")
    assert not missing, missing


def test_census_d_mbaff_neighbours():
    """On every V3, V4 and H2 edge the two neighbour MBs gave different (alpha, beta) or a different bS
    to the luma lines of that one edge, so the choice of neighbour per line or per field edge shows."""
    edges = {}
    for _, _, log in _mbaff_walk():
        for pi, pl, vertical, cls, pa, bS, al, be, tc0, line, coords in log:
            if pl == 0 and cls[:2] in ("V3", "V4", "H2"):
                q0 = coords[4]
                key = (pi, cls[:2], q0[1] // 16, q0[0] // 16 if cls[:2] != "V4" else q0[0] // 32 * 2 + (q0[0] & 1))
                edges.setdefault(key, {}).setdefault(pa, []).append((al, be, bS))
    assert len(edges) >= 30
    for key, by in edges.items():
        assert len(by) == 2, (key, list(by))
        a, b = by.values()
        assert sorted(a) != sorted(b), (key, by)


@pytest.mark.parametrize("wrong", D2.WRONG_MBAFF)
def test_d_mbaff_mutation(wrong):
    """A deliberately wrong MBAFF restatement differs from the oracle's output on some picture."""
    c = X.build("d_mbaff")
    for pi, (full, _, _) in enumerate(_mbaff_walk()):
        planes = D2.restate_mbaff(c, pi, wrong=(wrong,))
        if any(not np.array_equal(planes[k], full[k]) for k in range(3)):
            return
    raise AssertionError(f"d_mbaff: the restatement with {wrong} equals the oracle on every picture")
