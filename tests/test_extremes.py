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
import extremes_i as I
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
