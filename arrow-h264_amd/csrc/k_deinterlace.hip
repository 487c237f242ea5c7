// k_deinterlace.hip -- the deinterlacer of include/h264r_deinterlace.h (its comment is the definition; the
// names below are the header's): whole progressive pictures from the fields of the frame table, one launch
// for every job and plane of a call, nothing but registers.
//
// The unit of work is DEINT_UNIT = 16 adjacent columns of one field row m of a plane's cropped rectangle:
// a lane writes the kept row 2 m + keep and the interpolated row 2 m + q of its columns, 16 bytes each.
// A workgroup is one wave and owns a tile of DEINT_TW x DEINT_TH samples: two units side by side, 32 field
// rows.  What a lane loads is exactly what the definition names for its 16 columns: the rows ia, ib of K
// with 4 more bytes on either side (S and pr reach 3 columns out), the rows ia, ib of Pb and Pa, the rows
// mu, m, md of Qb and Qa -- 16 unaligned 16-byte loads and 4 dwords; rows that clamp load the same address
// twice.  In a tile that has whole tiles on both sides (wave-uniform, a scalar branch) every load is one
// instruction; in the first and the last tile of a row of tiles the halo outside the rectangle repeats the
// edge sample and a unit cut by the right edge is fetched bytewise with the clamp, so nothing outside the
// crop is read.  Either way the rows then sit in the same registers and go through the same arithmetic.
//
// Arithmetic: packed pairs of 16-bit values (v_pk_*), two pixels an instruction; a dword of 4 samples is
// taken apart as samples 0, 2 and samples 1, 3 (one v_perm_b32 each, which also shifts the row by j for
// pr(j)).  Everything the definition computes stays within +-765.  S(j) is one v_sad_u8 per pixel over two
// v_perm_b32 that pick its three bytes of either row.  Comparisons are the sign of a packed difference,
// selections v_bfi_b32.  BOB is the rounded-up byte average of the two rows, on whole dwords.
//
// A full unit leaves as one 16-byte store (global_store_dwordx4 has no alignment requirement on gfx950, as
// the loads have none), a unit cut by the right edge bytewise: never a byte outside the rectangle.
//
// Grid: x = tiles of the plane with the most, rounded up to DEINT_GROUP and permuted by deint_tile();
// job z / nplanes * grid.y + y, so that one launch holds any number; plane z % nplanes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "output_rgb.h"   // the unaligned loads

namespace h264r {

typedef uint32_t u32_u __attribute__((aligned(1)));
typedef int16_t v2s __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t ld4u(const uint8_t* p) { return *(const H264R_GLOBAL u32_u*)p; }

// One source of a job, as this block's plane sees it.
struct DeintSrc {
    int kind;
    const uint8_t *p0, *p1;
};

// a or b, member by member: the sources stay in registers
__device__ __forceinline__ DeintSrc deint_either(bool first, const DeintSrc& a, const DeintSrc& b)
{
    DeintSrc r;
    r.kind = first ? a.kind : b.kind;
    r.p0 = first ? a.p0 : b.p0;
    r.p1 = first ? a.p1 : b.p1;
    return r;
}

// One field of a source: row m of the cropped rectangle starts at p + m * stride.
struct DeintField {
    const uint8_t* p;
    int64_t stride;
};

// Entry idx of the frame table: its kind and planes tested (every plane, so that the blocks of all planes
// agree), this plane's pointers returned.  unpaired: the parity an unpaired field may have, -1: none.
__device__ __forceinline__ bool deint_source(const h264r_out_frame* __restrict__ frames, int idx, int need_chroma, int which,
                                             int unpaired, DeintSrc& s)
{
    const int kind = frames[idx].kind;
    const bool pair = kind == H264R_OUT_FIELD_PAIR;
    bool ok = kind == H264R_OUT_FRAME || pair || (unpaired >= 0 && kind == H264R_OUT_UNPAIRED_TOP + unpaired);
    const uint8_t* const y0 = frames[idx].y[0];
    const uint8_t* const y1 = frames[idx].y[1];
    ok = ok && y0 && (!pair || y1);
    s.kind = kind;
    s.p0 = y0; s.p1 = y1;
    if (need_chroma) {
        const uint8_t* const u0 = frames[idx].u[0];
        const uint8_t* const u1 = frames[idx].u[1];
        const uint8_t* const v0 = frames[idx].v[0];
        const uint8_t* const v1 = frames[idx].v[1];
        ok = ok && u0 && v0 && (!pair || (u1 && v1));
        if (which == 1) { s.p0 = u0; s.p1 = u1; }
        if (which == 2) { s.p0 = v0; s.p1 = v1; }
    }
    return ok;
}

__device__ __forceinline__ DeintField deint_field(const DeintSrc& s, int parity, const DeintPlane& P)
{
    DeintField f;
    if (s.kind == H264R_OUT_FRAME) {
        f.p = s.p0 + (int64_t)(P.y0 + parity) * P.pitch + P.x0;
        f.stride = 2 * (int64_t)P.pitch;
    } else {
        f.p = (s.kind == H264R_OUT_FIELD_PAIR && parity ? s.p1 : s.p0) + (int64_t)(P.y0 >> 1) * P.pitch + P.x0;
        f.stride = P.pitch;
    }
    return f;
}

// Columns x .. x + 15 of a row of w samples; EDGE: those at and behind w repeat sample w - 1 (x < w).
template <bool EDGE>
__device__ __forceinline__ void deint_row16(const uint8_t* r, int x, int w, uint32_t (&c)[4])
{
    if (!EDGE || x + DEINT_UNIT <= w) {
        const uint4 v = ld16u(r + x);
        c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) v |= (uint32_t)ld1(r + min(x + 4 * i + b, w - 1)) << (8 * b);
        c[i] = v;
    }
}

// Columns x - 4 .. x + 19: E[1 .. 4] the unit, E[0] and E[5] the halo, clamped to 0 .. w - 1 under EDGE.
template <bool EDGE>
__device__ __forceinline__ void deint_row24(const uint8_t* r, int x, int w, uint32_t (&E)[6])
{
    uint32_t c[4];
    deint_row16<EDGE>(r, x, w, c);
    E[1] = c[0]; E[2] = c[1]; E[3] = c[2]; E[4] = c[3];
    if (!EDGE) {
        E[0] = ld4u(r + x - 4);
        E[5] = ld4u(r + x + DEINT_UNIT);
        return;
    }
    E[0] = x > 0 ? ld4u(r + x - 4) : (c[0] & 0xffu) * 0x01010101u;
    if (x + DEINT_UNIT + 4 <= w) {
        E[5] = ld4u(r + x + DEINT_UNIT);
    } else {
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) v |= (uint32_t)ld1(r + min(x + DEINT_UNIT + i, w - 1)) << (8 * i);
        E[5] = v;
    }
}

// bytes p, p + 1, p + 2 of the 24-byte row E and a zero: what v_sad_u8 sums for one pixel
__device__ __forceinline__ uint32_t deint_pick3(const uint32_t (&E)[6], int p)
{
    const int k = p >> 2, o = p & 3;
    const uint32_t sel = (uint32_t)o | (uint32_t)(o + 1) << 8 | (uint32_t)(o + 2) << 16 | 0x0c000000u;
    return __builtin_amdgcn_perm(E[k < 5 ? k + 1 : 5], E[k], sel);
}

// bytes p and p + 2 of the 24-byte row E as a pair of 16-bit values
__device__ __forceinline__ v2s deint_pick2(const uint32_t (&E)[6], int p)
{
    const int k = p >> 2, o = p & 3;
    const uint32_t sel = (uint32_t)o | 0x0c00u | (uint32_t)(o + 2) << 16 | 0x0c000000u;
    return __builtin_bit_cast(v2s, __builtin_amdgcn_perm(E[k < 5 ? k + 1 : 5], E[k], sel));
}

// bytes h and h + 2 of a dword as a pair of 16-bit values
__device__ __forceinline__ v2s deint_pair(uint32_t w, int h)
{
    return __builtin_bit_cast(v2s, (w >> (8 * h)) & 0x00ff00ffu);
}

__device__ __forceinline__ v2s deint_max(v2s a, v2s b) { return __builtin_elementwise_max(a, b); }
__device__ __forceinline__ v2s deint_min(v2s a, v2s b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ v2s deint_absdiff(v2s a, v2s b) { return deint_max(a, b) - deint_min(a, b); }
// all ones where a < b: both within +-16383
__device__ __forceinline__ v2s deint_lt(v2s a, v2s b) { return (a - b) >> 15; }
__device__ __forceinline__ v2s deint_sel(v2s m, v2s a, v2s b) { return (a & m) | (b & ~m); }

// S(j) of the pixels xl and xl + 2 of the unit
__device__ __forceinline__ v2s deint_score(const uint32_t (&A)[6], const uint32_t (&B)[6], int xl, int j)
{
    const uint32_t s0 = __builtin_amdgcn_sad_u8(deint_pick3(A, 3 + xl + j), deint_pick3(B, 3 + xl - j), 0u);
    const uint32_t s1 = __builtin_amdgcn_sad_u8(deint_pick3(A, 5 + xl + j), deint_pick3(B, 5 + xl - j), 0u);
    return __builtin_bit_cast(v2s, s0 | s1 << 16);
}

// One direction of the edge search: s, and 2 s only where s was taken.
__device__ __forceinline__ void deint_search(const uint32_t (&A)[6], const uint32_t (&B)[6], int xl, int s, v2s& score, v2s& sp)
{
    const v2s s1 = deint_score(A, B, xl, s);
    const v2s m1 = deint_lt(s1, score);
    score = deint_sel(m1, s1, score);
    sp = deint_sel(m1, (deint_pick2(A, 4 + xl + s) + deint_pick2(B, 4 + xl - s)) >> 1, sp);
    const v2s s2 = deint_score(A, B, xl, 2 * s);
    const v2s m2 = deint_lt(s2, score) & m1;
    score = deint_sel(m2, s2, score);
    sp = deint_sel(m2, (deint_pick2(A, 4 + xl + 2 * s) + deint_pick2(B, 4 + xl - 2 * s)) >> 1, sp);
}

// The rows an ADAPTIVE unit needs, as the loads left them.
struct DeintRows {
    uint32_t A[6], B[6];              // K[ia], K[ib], columns x - 4 .. x + 19
    uint32_t pbA[4], pbB[4];          // Pb[ia], Pb[ib]
    uint32_t paA[4], paB[4];          // Pa[ia], Pa[ib]
    uint32_t qb[3][4], qa[3][4];      // Qb, Qa at mu, m, md
};

// The interpolated row of one unit.
__device__ __forceinline__ void deint_adaptive(const DeintRows& R, uint32_t (&out)[4])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t word = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int xl = 4 * i + h;                         // the pair: pixels xl and xl + 2
            const v2s c = deint_pair(R.A[1 + i], h), e = deint_pair(R.B[1 + i], h);
            const v2s qbm = deint_pair(R.qb[1][i], h), qam = deint_pair(R.qa[1][i], h);
            const v2s d = (qbm + qam) >> 1;
            const v2s t0 = deint_absdiff(qbm, qam) >> 1;
            const v2s t1 = (deint_absdiff(deint_pair(R.pbA[i], h), c) + deint_absdiff(deint_pair(R.pbB[i], h), e)) >> 1;
            const v2s t2 = (deint_absdiff(deint_pair(R.paA[i], h), c) + deint_absdiff(deint_pair(R.paB[i], h), e)) >> 1;
            v2s diff = deint_max(t0, deint_max(t1, t2));

            v2s sp = (c + e) >> 1;
            v2s score = deint_score(R.A, R.B, xl, 0) - (v2s)(1);
            deint_search(R.A, R.B, xl, -1, score, sp);
            deint_search(R.A, R.B, xl, 1, score, sp);

            const v2s b = (deint_pair(R.qb[0][i], h) + deint_pair(R.qa[0][i], h)) >> 1;
            const v2s f = (deint_pair(R.qb[2][i], h) + deint_pair(R.qa[2][i], h)) >> 1;
            const v2s de = d - e, dc = d - c, bc = b - c, fe = f - e;
            const v2s mx = deint_max(deint_max(de, dc), deint_min(bc, fe));
            const v2s mn = deint_min(deint_min(de, dc), deint_max(bc, fe));
            diff = deint_max(diff, deint_max(mn, -mx));
            const v2s o = deint_min(deint_max(sp, d - diff), d + diff);
            word |= __builtin_bit_cast(uint32_t, o) << (8 * h);
        }
        out[i] = word;
    }
}

// n bytes of a unit to d: all 16 as one store, which like the loads needs no alignment; fewer bytewise
__device__ __forceinline__ void deint_store(uint8_t* d, uint4 v, int n)
{
    if (n == DEINT_UNIT) {
        u32x4 t;
        t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
        *(H264R_GLOBAL u32x4_u*)d = t;
    } else {
        // the bytes that are left, last dword first: a shift a byte, no index into the unit
        uint64_t lo = v.x | (uint64_t)v.y << 32, hi = v.z | (uint64_t)v.w << 32;
#pragma unroll 1
        for (int b = 0; b < n; ++b) {
            d[b] = (uint8_t)lo;
            lo = lo >> 8 | hi << 56;
            hi >>= 8;
        }
    }
}

// What a good job resolves to for this block's plane.
struct DeintWork {
    DeintField K, Pb, Pa, Qb, Qa;     // BOB: K alone
    int keep, mode;
};

template <bool EDGE>
__device__ __forceinline__ void deint_unit(const DeintWork& W, const DeintPlane& P, int x, int m, uint8_t* fdst)
{
    const int Hf = P.h >> 1, w = P.w;
    const int q = 1 - W.keep;
    const int ia = min(max(m + q - 1, 0), Hf - 1), ib = min(m + q, Hf - 1);
    uint32_t kept[4], out[4];
    if (W.mode == H264R_DEINT_BOB) {
        uint32_t a[4], b[4];
        deint_row16<EDGE>(W.K.p + ia * W.K.stride, x, w, a);
        deint_row16<EDGE>(W.K.p + ib * W.K.stride, x, w, b);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            out[i] = (a[i] | b[i]) - (((a[i] ^ b[i]) >> 1) & 0x7f7f7f7fu);     // (c + e + 1) >> 1 of every byte
            kept[i] = q ? a[i] : b[i];
        }
    } else {
        const int mu = max(m - 1, 0), md = min(m + 1, Hf - 1);
        DeintRows R;
        deint_row24<EDGE>(W.K.p + ia * W.K.stride, x, w, R.A);
        deint_row24<EDGE>(W.K.p + ib * W.K.stride, x, w, R.B);
        deint_row16<EDGE>(W.Pb.p + ia * W.Pb.stride, x, w, R.pbA);
        deint_row16<EDGE>(W.Pb.p + ib * W.Pb.stride, x, w, R.pbB);
        deint_row16<EDGE>(W.Pa.p + ia * W.Pa.stride, x, w, R.paA);
        deint_row16<EDGE>(W.Pa.p + ib * W.Pa.stride, x, w, R.paB);
        const int rows[3] = {mu, m, md};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            deint_row16<EDGE>(W.Qb.p + rows[k] * W.Qb.stride, x, w, R.qb[k]);
            deint_row16<EDGE>(W.Qa.p + rows[k] * W.Qa.stride, x, w, R.qa[k]);
        }
        deint_adaptive(R, out);
#pragma unroll
        for (int i = 0; i < 4; ++i) kept[i] = q ? R.A[1 + i] : R.B[1 + i];
    }
    const int n = min(DEINT_UNIT, w - x);
    uint8_t* const d = fdst + (int64_t)(P.y0 + 2 * m) * P.pitch + P.x0 + x;
    deint_store(d + (int64_t)W.keep * P.pitch, make_uint4(kept[0], kept[1], kept[2], kept[3]), n);
    deint_store(d + (int64_t)q * P.pitch, make_uint4(out[0], out[1], out[2], out[3]), n);
}

}  // namespace h264r

using namespace h264r;

extern "C" __global__ void __launch_bounds__(DEINT_THREADS)
k_deinterlace(DeintJob job, const h264r_out_frame* __restrict__ frames, const h264r_deint_job* __restrict__ jobs, uint8_t* dst,
              int* err)
{
    const int pl = (int)blockIdx.z % job.nplanes;
    const int j = (int)blockIdx.z / job.nplanes * (int)gridDim.y + (int)blockIdx.y;
    if (j >= job.num_jobs) return;
    const DeintPlane P = job.pl[pl];
    const int tile = deint_tile((int)blockIdx.x);
    if (tile >= P.tiles) return;
    const int ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
    const int lane = (int)threadIdx.x;
    const int x = tx * DEINT_TW + (lane & 1) * DEINT_UNIT;
    const int m = ty * (DEINT_TH / 2) + (lane >> 1);
    const bool active = x < P.w && m < (P.h >> 1);
    // whole tiles on both sides: every halo is inside the rectangle
    const bool interior = tx > 0 && (tx + 1) * DEINT_TW + 4 <= P.w;
    const int n = job.num_frames;

    {
        // the refusals: the record's rule, then the sources, before any plane pointer is used
        const int cur = jobs[j].cur, prev = jobs[j].prev, next = jobs[j].next;
        const int keep = jobs[j].keep, second = jobs[j].second, mode = jobs[j].mode;
        bool ok = (unsigned)cur < (unsigned)n && prev >= -1 && prev < n && next >= -1 && next < n && (unsigned)keep <= 1u &&
                  (unsigned)second <= 1u && (mode == H264R_DEINT_BOB || mode == H264R_DEINT_ADAPTIVE);
        DeintWork W;
        W.keep = keep; W.mode = mode;
        if (ok) {
            DeintSrc C;
            ok = deint_source(frames, cur, job.need_chroma, P.which, mode == H264R_DEINT_BOB ? keep : -1, C);
            if (ok) W.K = deint_field(C, keep, P);
            if (ok && mode == H264R_DEINT_ADAPTIVE) {
                // prev / next == -1: cur, which has passed
                DeintSrc Ps, Ns;
                ok = deint_source(frames, prev >= 0 ? prev : cur, job.need_chroma, P.which, -1, Ps);
                ok = deint_source(frames, next >= 0 ? next : cur, job.need_chroma, P.which, -1, Ns) && ok;
                if (ok) {
                    const int q = 1 - keep;
                    W.Pb = deint_field(Ps, keep, P);
                    W.Pa = deint_field(Ns, keep, P);
                    W.Qb = deint_field(deint_either(second, C, Ps), q, P);
                    W.Qa = deint_field(deint_either(second, Ns, C), q, P);
                }
            }
        }
        if (!ok) {
            if (blockIdx.x == 0 && pl == 0 && lane == 0) atomicOr(err, DEV_ERR_OUTPUT);
            return;
        }
        if (!active) return;
        uint8_t* const fdst = dst + (int64_t)j * job.frame_stride + P.off;
        if (interior) deint_unit<false>(W, P, x, m, fdst);
        else deint_unit<true>(W, P, x, m, fdst);
    }
}
