// Rotated-rectangle clipping shared by nms.hip (rotated IoU matrix, NMS) and kitti_eval.hip (per-image BEV overlaps): the fp32
// polygon-clipping arithmetic of second/core/non_max_suppression/nms_gpu.py:166-401, operation for operation (compiled with
// -ffp-contract=off).  Moved here from nms.hip unchanged.
#pragma once
#include "common.hpp"

namespace sec {

__device__ __forceinline__ float tri_area(const float *a, const float *b, const float *c) {
    return ((a[0] - c[0]) * (b[1] - c[1]) - (a[1] - c[1]) * (b[0] - c[0])) / 2.0f;
}

__device__ __forceinline__ void box_corners(float *c, const float *b) {  // nms_gpu.py:353-376
    float ac = cosf(b[4]), as = sinf(b[4]);
    float cx = b[0], cy = b[1], xd = b[2], yd = b[3];
    float xs[4] = {-xd / 2, -xd / 2, xd / 2, xd / 2};
    float ys[4] = {-yd / 2, yd / 2, yd / 2, -yd / 2};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c[2 * i] = ac * xs[i] + as * ys[i] + cx;
        c[2 * i + 1] = -as * xs[i] + ac * ys[i] + cy;
    }
}

__device__ __forceinline__ bool pt_in_quad(float x, float y, const float *c) {  // nms_gpu.py:308-325
    float ab0 = c[2] - c[0], ab1 = c[3] - c[1];
    float ad0 = c[6] - c[0], ad1 = c[7] - c[1];
    float ap0 = x - c[0], ap1 = y - c[1];
    float abab = ab0 * ab0 + ab1 * ab1;
    float abap = ab0 * ap0 + ab1 * ap1;
    float adad = ad0 * ad0 + ad1 * ad1;
    float adap = ad0 * ap0 + ad1 * ap1;
    const float eps = -1e-6f;
    return abab - abap >= eps && abap >= eps && adad - adap >= eps && adap >= eps;
}

__device__ __forceinline__ bool seg_intersect(const float *p1, const float *p2, int i, int j, float *t) {  // :222-264
    float A0 = p1[2 * i], A1 = p1[2 * i + 1];
    float B0 = p1[2 * ((i + 1) & 3)], B1 = p1[2 * ((i + 1) & 3) + 1];
    float C0 = p2[2 * j], C1 = p2[2 * j + 1];
    float D0 = p2[2 * ((j + 1) & 3)], D1 = p2[2 * ((j + 1) & 3) + 1];
    float BA0 = B0 - A0, BA1 = B1 - A1, DA0 = D0 - A0, CA0 = C0 - A0, DA1 = D1 - A1, CA1 = C1 - A1;
    bool acd = DA1 * CA0 > CA1 * DA0;
    bool bcd = (D1 - B1) * (C0 - B0) > (C1 - B1) * (D0 - B0);
    if (acd != bcd) {
        bool abc = CA1 * BA0 > BA1 * CA0;
        bool abd = DA1 * BA0 > BA1 * DA0;
        if (abc != abd) {
            float DC0 = D0 - C0, DC1 = D1 - C1;
            float ABBA = A0 * B1 - B0 * A1;
            float CDDC = C0 * D1 - D0 * C1;
            float DH = BA1 * DC0 - BA0 * DC1;
            float Dx = ABBA * DC0 - BA0 * CDDC;
            float Dy = ABBA * DC1 - BA1 * CDDC;
            t[0] = Dx / DH;
            t[1] = Dy / DH;
            return true;
        }
    }
    return false;
}

// intersection area of two quads given by their corners (nms_gpu.py:329-350,172-219,379-393)
// The reference indexes its vertex list dynamically (append, insertion sort).  In registers that means scratch memory, in LDS
// (rounds 1-2) a ~100-clock round trip per access on a serial chain of a few hundred accesses: ~18 us per clip with one wave per
// SIMD, and a launch lasts as long as its slowest clip.  Here the list (at most 8 vertices are ever used -- the reference's
// int_pts holds 8; later ones are counted, not stored) lives in registers and every index is static: an append is eight selects
// on "n == slot", the insertion sort is unrolled with a `moving` predicate that replays the reference's while loop step by step
// (same comparisons in the same order, so ties and NaN keys fall exactly where the reference's sort leaves them), the centroid
// and the triangle fan run to 8 / 6 with "i < n" predicates.  No LDS, no data-dependent branches except the per-edge-pair
// "these two segments cross" block.
__device__ __forceinline__ void vl_append(float (&px)[8], float (&py)[8], int &n, bool hit, float vx, float vy) {
#pragma unroll
    for (int sl = 0; sl < 8; ++sl) {
        const bool wr = hit && n == sl;
        px[sl] = wr ? vx : px[sl];
        py[sl] = wr ? vy : py[sl];
    }
    n += hit ? 1 : 0;
}

__device__ float quad_inter(const float (&c1)[8], const float (&c2)[8]) {
    float px[8], py[8], key[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) px[i] = py[i] = key[i] = 0.0f;
    int n = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        vl_append(px, py, n, pt_in_quad(c1[2 * i], c1[2 * i + 1], c2), c1[2 * i], c1[2 * i + 1]);
        vl_append(px, py, n, pt_in_quad(c2[2 * i], c2[2 * i + 1], c1), c2[2 * i], c2[2 * i + 1]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float t[2] = {0.0f, 0.0f};
            const bool hit = seg_intersect(c1, c2, i, j, t);
            vl_append(px, py, n, hit, t[0], t[1]);
        }
    if (n > 8) n = 8;
    if (n < 3) return 0.0f;
    // angular sort about the centroid (insertion sort on the reference's key)
    float cx = 0.0f, cy = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        cx = i < n ? cx + px[i] : cx;
        cy = i < n ? cy + py[i] : cy;
    }
    cx /= (float)n;
    cy /= (float)n;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float vx = px[i] - cx, vy = py[i] - cy;
        float d = sqrtf(vx * vx + vy * vy);
        vx = vx / d;
        vy = vy / d;
        if (vy < 0) vx = -2 - vx;
        key[i] = vx;                        // slots >= n are never compared (every step below is predicated on i < n)
    }
#pragma unroll
    for (int i = 1; i < 8; ++i) {
        // reference: if (V[i-1] > V[i]) { temp = V[i]; j = i; while (j > 0 && V[j-1] > temp) { V[j] = V[j-1]; --j; } V[j] = temp; }
        const float temp = key[i], tx = px[i], ty = py[i];
        bool moving = i < n && key[i - 1] > temp;
#pragma unroll
        for (int j = i; j >= 1; --j) {
            const bool shift = moving && key[j - 1] > temp;
            key[j] = shift ? key[j - 1] : (moving ? temp : key[j]);
            px[j] = shift ? px[j - 1] : (moving ? tx : px[j]);
            py[j] = shift ? py[j - 1] : (moving ? ty : py[j]);
            moving = shift;
        }
        key[0] = moving ? temp : key[0];
        px[0] = moving ? tx : px[0];
        py[0] = moving ? ty : py[0];
    }
    float s = 0.0f;
    const float p0[2] = {px[0], py[0]};
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float pa[2] = {px[i + 1], py[i + 1]}, pb[2] = {px[i + 2], py[i + 2]};
        const float a = fabsf(tri_area(p0, pa, pb));
        s = i < n - 2 ? s + a : s;
    }
    return s;
}

struct Standup { float x0, y0, x1, y1; };
__device__ __forceinline__ Standup standup_of(const float *c) {
    Standup s{c[0], c[1], c[0], c[1]};
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        s.x0 = fminf(s.x0, c[2 * i]); s.x1 = fmaxf(s.x1, c[2 * i]);
        s.y0 = fminf(s.y0, c[2 * i + 1]); s.y1 = fmaxf(s.y1, c[2 * i + 1]);
    }
    return s;
}
// far apart => the clipper finds no vertex => intersection exactly 0 (margin covers its 1e-6 tolerances) -- for boxes that are not
// thin_box(), see there
__device__ __forceinline__ bool far_apart(const Standup &a, const Standup &b) {
    const float m = 1e-3f;
    return a.x0 > b.x1 + m || b.x0 > a.x1 + m || a.y0 > b.y1 + m || b.y0 > a.y1 + m;
}
// pt_in_quad's tolerance is 1e-6 on DOT PRODUCTS with the edge vectors, i.e. a distance of 1e-6 / side: a box with a side of 1e-4
// "contains" points 1 cm outside it, and one with a zero side every point of the strip (zero area: of the plane) its other side
// spans -- the reference then reports the far box's own corners as the intersection and suppresses it (IoU = area / 0).  far_apart's
// 1 mm margin covers that tolerance down to sides of 2 mm; a thinner box goes through the clipper whatever its distance.
__device__ __forceinline__ bool thin_box(const float *b) { return !(fminf(fabsf(b[2]), fabsf(b[3])) >= 2e-3f); }

}  // namespace sec
