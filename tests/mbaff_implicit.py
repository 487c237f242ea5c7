"""Helpers of the MBAFF implicit-weight tests (test_mbaff_implicit.py, test_gpu_mbaff_implicit.py).

Neither the reference driver nor the CPU oracle decodes a field MB with implicit weights in an MBAFF
frame, so the expected samples are assembled from parts the oracle does
decode and the reference pins:

  field MBs   An inter MB's reconstruction depends on no other MB, so the field MB of parity a in
              pair row r is MB (x, r) of a FIELD PICTURE of parity a made of the same records, levels
              and motion (`field_picture`): its lists are the MBAFF lists with every entry doubled
              into (same parity, other parity), its implicit_w1 table is filled by `w1_rule`, the
              Python restatement of inter_prediction.cc:120-137, from the h264r_field_poc record.
  the rest    The same MBAFF picture with list 1 removed from every bi-predicted block of a field
              MB (`strip_field_bipred`): the oracle decodes it with wp_mode 2 (frame MBs take the
              slice's table; single-list blocks are not weighted).
  filtering   oracle_deblock_picture on the assembled reconstruction (it does not predict).

Intra MBs read their neighbours' reconstruction, so the pictures are intra-free or use
constrained_intra_pred, under which an intra MB never reads an inter MB.
"""
import ctypes as C

import numpy as np

import _oracle as O
from h264r import _abi as A
from h264r import synth


def clip3(lo, hi, x):
    return lo if x < lo else hi if x > hi else x


def cdiv(a, b):
    """C's truncating integer division."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def w1_rule(cur, poc0, poc1, lt0=0, lt1=0):
    """weight1 of bi_prediction (inter_prediction.cc:120-137), restated."""
    td = clip3(-128, 127, poc1 - poc0)
    if td == 0 or lt0 or lt1:
        return 32
    tb = clip3(-128, 127, cur - poc0)
    tx = cdiv(16384 + abs(cdiv(td, 2)), td)
    w1 = clip3(-1024, 1023, (tx * tb + 32) >> 6) >> 2
    return 32 if w1 < -64 or w1 > 128 else w1


def record(L, p, cur=None):
    """The generator's DPB as an h264r_field_poc record, current POCs (poc, poc + 1) by default."""
    rec = synth.field_pocs(L, p)
    poc = int(p.pic["poc"][0])
    rec["cur_poc"][0] = (poc, poc + 1) if cur is None else cur
    return rec


def clone(p):
    return synth.Picture(A.SynthCfg.from_dict(p.cfg.as_dict()), p.index, p.mbs.copy(), p.levels.copy(), p.mv.copy(),
                         p.ref_idx.copy(), p.slices.copy(), p.pic.copy())


def field_mb_mask(p):
    """[H, W] bool: inter MBs coded as field MBs."""
    f = p.mbs["flags"].reshape(p.cfg.height_mbs, p.cfg.width_mbs)
    return ((f & A.MBF_FIELD) != 0) & ((f & A.MBF_INTRA) == 0)


def block_mask(p):
    """[4H, 4W] bool: 4x4 blocks of field inter MBs predicted from both lists."""
    m = np.repeat(np.repeat(field_mb_mask(p), 4, 0), 4, 1)
    return m & (p.ref_idx[0] >= 0) & (p.ref_idx[1] >= 0)


def frame_table(p, rec):
    """implicit_w1 of the frame MBs: the frame POCs (a frame's POC is the smaller of its fields')."""
    poc = int(p.pic["poc"][0])
    for sl in p.slices:
        for i0 in range(sl["num_ref"][0]):
            for i1 in range(sl["num_ref"][1]):
                s0, s1 = int(sl["ref_slot"][0][i0]), int(sl["ref_slot"][1][i1])
                sl["implicit_w1"][i0][i1] = w1_rule(poc, int(rec["slot_poc"][0, s0].min()), int(rec["slot_poc"][0, s1].min()))


def implicit_picture(p0, rec):
    """The wp_mode 0 MBAFF picture p0 with implicit weights: wp_mode 2 and the frame MBs' table."""
    p = clone(p0)
    p.slices["wp_mode"] = 2
    frame_table(p, rec)
    return p


def strip_field_bipred(p):
    """p with list 1 removed from every bi-predicted 4x4 block of a field MB."""
    q = clone(p)
    q.ref_idx[1][block_mask(p)] = -1
    return q


# the four wrong derivations of the evidence census, and the right one
VARIANTS = ("right", "swapped_parity", "frame_pocs", "other_cur")


def field_picture(p, a, rec=None, variant="right"):
    """The field picture of parity a holding p's MB rows a::2 (module docstring).  With wp_mode 2 its
    implicit_w1 table comes from rec by w1_rule; `variant` names a deliberately wrong derivation."""
    W, H = p.cfg.width_mbs, p.cfg.height_mbs
    cfg = A.SynthCfg.from_dict(p.cfg.as_dict())
    cfg.structure, cfg.height_mbs = A.TOP_FIELD + a, H // 2
    mbs = p.mbs.reshape(H, W)[a::2].reshape(-1).copy()
    mbs["flags"] &= ~np.uint8(A.MBF_FIELD)
    mv = np.ascontiguousarray(p.mv.reshape(2, H, 4, 4 * W)[:, a::2].reshape(2, 2 * H, 4 * W))
    rr = np.ascontiguousarray(p.ref_idx.reshape(2, H, 4, 4 * W)[:, a::2].reshape(2, 2 * H, 4 * W))
    slices = p.slices.copy()
    pic = p.pic.copy()
    pic["structure"] = A.TOP_FIELD + a
    for k, src in enumerate(p.slices):
        sl = slices[k]
        n = [int(src["num_ref"][0]), int(src["num_ref"][1])]
        assert max(n) <= 8
        sl["num_ref"] = (2 * n[0], 2 * n[1])
        ent = [[], []]                                   # (slot, bottom) of every doubled entry
        for l in range(2):
            sl["ref_slot"][l] = -1
            for i in range(2 * n[l]):
                slot, bot = int(src["ref_slot"][l][i >> 1]), int((i & 1) != a)
                sl["ref_slot"][l][i] = slot | (A.REF_BOTTOM if bot else 0)
                sl["wp_weight"][l][i] = src["wp_weight"][l][i >> 1]
                sl["wp_offset"][l][i] = src["wp_offset"][l][i >> 1]
                ent[l].append((slot, bot))
        if int(src["wp_mode"]) != 2:
            continue

        def poc_lt(slot, bot):
            if variant == "swapped_parity":
                bot = 1 - bot
            if variant == "frame_pocs":
                return int(rec["slot_poc"][0, slot].min()), 0
            return int(rec["slot_poc"][0, slot, bot]), int(rec["long_term"][0, bot] >> slot) & 1

        cur = int(rec["cur_poc"][0, 1 - a if variant == "other_cur" else a])
        if variant == "frame_pocs":
            cur = int(rec["cur_poc"][0].min())
        sl["implicit_w1"] = 0
        for i0, e0 in enumerate(ent[0]):
            for i1, e1 in enumerate(ent[1]):
                (p0, t0), (p1, t1) = poc_lt(*e0), poc_lt(*e1)
                sl["implicit_w1"][i0][i1] = w1_rule(cur, p0, p1, t0, t1)
    return synth.Picture(cfg, p.index, mbs, p.levels, mv, rr, slices, pic)


def field_recons(p, refs, rec=None, variant="right"):
    """The reconstructions of the two derived field pictures, [parity] -> (Y, Cb, Cr)."""
    return [O.decode(field_picture(p, a, rec, variant), refs, stage="recon") for a in range(2)]


def paste_field_mbs(p, planes, fields):
    """Write every field inter MB of p from the derived field pictures' reconstructions into the
    frame planes: frame row 32 r + a + 2 k of the pair row r is row 16 r + k of field a."""
    fm = field_mb_mask(p)
    for y, x in np.argwhere(fm):
        r, a = y >> 1, y & 1
        for k, n in ((0, 16), (1, 8), (2, 8)):
            planes[k][2 * n * r + a:2 * n * (r + 1):2, n * x:n * (x + 1)] = \
                fields[a][k][n * r:n * (r + 1), n * x:n * (x + 1)]


def expect_recon(p, refs, rec=None, variant="right"):
    """The assembled reconstruction (before the loop filter) of MBAFF picture p."""
    planes = O.decode(strip_field_bipred(p), refs, stage="recon")
    paste_field_mbs(p, planes, field_recons(p, refs, rec, variant))
    return planes


def deblock(p, refs, planes):
    """oracle_deblock_picture of p on a copy of `planes`."""
    out = tuple(np.ascontiguousarray(a).copy() for a in planes)
    q = O.quant_flat()
    o = O.make_oracle_picture(p, refs, q, out)
    st = O.lib().oracle_deblock_picture(C.byref(o))
    if st != 0:
        raise RuntimeError(f"oracle_deblock_picture -> {st}")
    return out


def expect(p, refs, rec=None, stage="full"):
    rc = expect_recon(p, refs, rec)
    return rc if stage == "recon" else deblock(p, refs, rc)


def field_mb_blocks(p, planes, a):
    """[n, 384] samples of the field inter MBs of parity a of frame planes, in raster order."""
    out = []
    for y, x in np.argwhere(field_mb_mask(p)):
        if (y & 1) != a:
            continue
        r = y >> 1
        out.append(np.concatenate([planes[k][2 * n * r + a:2 * n * (r + 1):2, n * x:n * (x + 1)].ravel()
                                   for k, n in ((0, 16), (1, 8), (2, 8))]))
    return np.array(out)


def differing_field_mbs(p, x, y, a):
    """How many field inter MBs of parity a differ between frame planes x and y."""
    bx, by = field_mb_blocks(p, x, a), field_mb_blocks(p, y, a)
    return int((bx != by).any(axis=1).sum()) if len(bx) else 0


# the pictures of the tests: config 4 (B), 22 x 18 MBs; (num_refs, index) of the three batch pictures
CASES = ((3, 0), (2, 1), (4, 2))


def mbaff_cfg(L, W=22, H=18, **over):
    over.setdefault("wp_mode", 0)
    return synth.default_cfg(L, 4, W, H, structure=A.MBAFF_FRAME, **over)


_cache = {}


def case(L, num_refs, index):
    """(picture with implicit weights, refs, record) of one batch picture; computed once, shared."""
    key = (num_refs, index)
    if key not in _cache:
        cfg = mbaff_cfg(L, intra_permille=0, num_refs=num_refs)
        p0 = synth.picture(L, cfg, index)
        rec = record(L, p0)
        _cache[key] = (implicit_picture(p0, rec), synth.refpics(L, cfg), rec)
    return _cache[key]


def cip_case(L):
    """The whole-pipeline picture: constrained intra prediction, a quarter intra MBs, 3 slices, every
    edge filtered."""
    if "cip" not in _cache:
        cfg = mbaff_cfg(L, constrained_intra=1, intra_permille=250, num_refs=3, num_slices=3, deblock_idc=0)
        p0 = synth.picture(L, cfg, 0)
        rec = record(L, p0)
        _cache["cip"] = (implicit_picture(p0, rec), synth.refpics(L, cfg), rec)
    return _cache["cip"]
