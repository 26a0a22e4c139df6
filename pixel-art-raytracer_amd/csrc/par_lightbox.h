// par_lightbox.h — where the pixels that start a shadow walk in one bin can lie, for the range cull of ranged lights
// (PAR_LIGHTS_RANGED, par_raytracer.h).
//
// The light kernel walks once per (start bin, light) pair of a screen column. A pixel of screen column (bx, by) whose
// shadow ray starts in depth bin bz has
//   x         in the column's B pixel columns:  bx * B <= x <= bx * B + B - 1;
//   s = y + z = H - row, row one of the column's B rows (alt:725-726): H - by * B - B + 1 <= s <= H - by * B;
//   z         in what the truncating division of alt:727 maps to bz: bz * B <= z <= bz * B + B - 1, and for bz = 0 also
//             -(B - 1) <= z < 0;
// and y = s - z: a slanted slab, a box in (x, s, z). The L1 distance from a light at (lx, ly, lz) to it is three gaps
// added up, in plain integers: with w = z - lz and v = s - (ly + lz) the y and z terms are |w| + |v - w|, which is |v|
// while w lies between 0 and v and grows by 2 per step outside. So the least is reached at the w nearest to 0 that z
// allows and the v nearest to that w that s allows: |w| + gap(w, the range of v).
// It is the exact minimum of the L1 length `len` over the slab's integer points (tests/test_light_range_cpu.py holds it
// to an enumeration), and `len` is an integer that fp32 holds exactly. A pixel is in range iff len < r: when the
// distance is >= r no pixel that starts in the bin is in range, and the pair's walk is of no use to anyone.
//
// A second, finer test uses what the column holds. Every pixel of the column comes from one of the slot records of the
// column's bins (alt:303-366): its x lies in the record's [px, px + ex), its s in (py + pz, py + ey + pz + ez], its z
// is pz + the sprite's depth at the texel (alt:360-361), within [pz + dmin, pz + dmax] for the least and largest depth
// of the sprite table. par_light_slab_clip cuts the bin's slab down to what one record can show in it; the pair is
// culled when every record's piece is empty or out of reach.
//
// Plain C++ for host and device: the kernels (par_kernels.hip) and the host program a test compiles
// (tests/lightbox_check.cpp) run these very functions.
#ifndef PAR_LIGHTBOX_H
#define PAR_LIGHTBOX_H

#if defined(__HIPCC__)
#define PAR_LIGHTBOX_FN __host__ __device__ inline
#else
#define PAR_LIGHTBOX_FN inline
#endif

struct par_light_slab {
    int x0, x1, s0, s1, z0, z1;  // inclusive; s = y + z
};

PAR_LIGHTBOX_FN par_light_slab par_light_slab_of(int B, int H, int bx, int by, int bz) {
    par_light_slab b;
    b.x0 = bx * B;
    b.x1 = bx * B + B - 1;
    b.s0 = H - by * B - B + 1;
    b.s1 = H - by * B;
    b.z0 = bz == 0 ? -(B - 1) : bz * B;
    b.z1 = bz * B + B - 1;
    return b;
}

PAR_LIGHTBOX_FN int par_light_gap(int v, int lo, int hi) { return v < lo ? lo - v : (v > hi ? v - hi : 0); }

// The L1 distance in (x, y, z) from (lx, ly, lz) to the slab's nearest integer point (0 inside it).
PAR_LIGHTBOX_FN int par_light_slab_l1(const par_light_slab& b, int lx, int ly, int lz) {
    const int w0 = b.z0 - lz, w1 = b.z1 - lz;
    const int w = w0 > 0 ? w0 : (w1 < 0 ? w1 : 0);  // the z offset nearest to 0
    const int ls = ly + lz;
    return par_light_gap(lx, b.x0, b.x1) + (w < 0 ? -w : w) + par_light_gap(w, b.s0 - ls, b.s1 - ls);
}

// The part of slab `b` that a slot record (position p, extent e) can show, for sprite depths in [dmin, dmax]. False when
// it is empty.
PAR_LIGHTBOX_FN bool par_light_slab_clip(const par_light_slab& b, int px, int py, int pz, int ex, int ey, int ez, int dmin,
                                         int dmax, par_light_slab* out) {
    out->x0 = px > b.x0 ? px : b.x0;
    out->x1 = px + ex - 1 < b.x1 ? px + ex - 1 : b.x1;
    out->s0 = py + pz + 1 > b.s0 ? py + pz + 1 : b.s0;
    out->s1 = py + ey + pz + ez < b.s1 ? py + ey + pz + ez : b.s1;
    out->z0 = pz + dmin > b.z0 ? pz + dmin : b.z0;
    out->z1 = pz + dmax < b.z1 ? pz + dmax : b.z1;
    return out->x0 <= out->x1 && out->s0 <= out->s1 && out->z0 <= out->z1;
}

#endif
