/*
 * par_types.h — plain-C data model shared by the C-ABI (par_raytracer.h), the CPU oracle and the HIP kernels.
 *
 * Every struct here is byte-for-byte layout compatible with the reference type it replaces, so a caller that
 * holds the reference's `Entities`, `Sprite`, `Pixel`, `Color` arrays can hand the same memory to this library.
 * Citations are `file:line` relative to the reference repository (spr = src/sprites.hpp, alt = src/alternative.cpp).
 */
#ifndef PAR_TYPES_H
#define PAR_TYPES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Sprite geometry is fixed by the reference: 20 texels wide (literal `20` at alt:330), 40 tall (spr:67-71). */
#define PAR_SPRITE_W 20
#define PAR_SPRITE_H 40
#define PAR_SPRITE_TEXELS (PAR_SPRITE_W * PAR_SPRITE_H)
/* Slots per hash bin, wrapping counter (`sparse_bin_size`, alt:131). */
#define PAR_SLOTS 8
/* Largest palette this build accepts (the reference ships 4 entries, spr:60-65). */
#define PAR_MAX_PALETTE 256
/* Palette-index plane value written for pixels no primitive covers. */
#define PAR_PALIDX_BACKGROUND 0xFF

/* `Color`, spr:5-17: RGBA8, channel order red,green,blue,alpha in memory. */
typedef struct par_color {
    uint8_t red, green, blue, alpha;
} par_color;

/* `Vector<float>`, spr:20-51. */
typedef struct par_vec3 {
    float x, y, z;
} par_vec3;

/* `Pixel`, spr:53-58: the 28-byte G-buffer texel. */
typedef struct par_pixel {
    par_vec3 normal;
    par_color color;
    int32_t y, z;
    int32_t entity_index;
} par_pixel;

/* `Sprite`, spr:67-71: 16 000 bytes; texel index = row * 20 + column. */
typedef struct par_sprite {
    int32_t color[PAR_SPRITE_TEXELS]; /* palette index */
    int32_t depth[PAR_SPRITE_TEXELS];
    par_vec3 normal[PAR_SPRITE_TEXELS];
} par_sprite;

/* `AABB`, alt:35-38,88: two `Point<short>` + 4 bytes of tail padding, 16-byte aligned. */
typedef struct par_aabb {
    int16_t px, py, pz; /* position */
    int16_t ex, ey, ez; /* extent   */
    int16_t pad_[2];
} par_aabb;

/* `Light`, alt:619-622. `radius` is not read, as in the reference, unless the context's light model is
 * PAR_LIGHTS_RANGED (par_set_light_model, par_raytracer.h): then a radius > 0 bounds and attenuates the light by the L1
 * distance, and a radius <= 0 leaves it unbounded. */
typedef struct par_light {
    int16_t x, y, z;
    int16_t radius;
} par_light;

/* The colour of a light (par_set_light_tints, par_raytracer.h; nothing in the reference): what its term of a covered
 * pixel's sum is multiplied by, channel by channel. White is {1, 1, 1}; a component above 1 makes a bright light. */
typedef struct par_light_tint { float r, g, b; } par_light_tint;

/* How par_outline_device (par_raytracer.h; nothing in the reference) draws a frame's outlines: the depth difference from
 * which an edge between two entities is a silhouette, and the 8.8 fixed-point factors a silhouette's and a crease's red,
 * green and blue are multiplied by (256 leaves a colour as it is, below darkens, above lightens). */
typedef struct par_outline_style {
    int32_t depth_step;        /* >= 1 */
    int32_t silhouette_scale;  /* 0..1024, 256 = unchanged */
    int32_t crease_scale;      /* 0..1024, 256 = unchanged */
} par_outline_style;

/* How par_present_device (par_raytracer.h) puts a frame or an index plane on a surface: nearest neighbour at an integer
 * scale, in the surface's byte order and row pitch (the reference's present, alt:774-788, at scale 1). */
#define PAR_MAX_SCALE 16
enum { PAR_PRESENT_RGBA = 0, PAR_PRESENT_BGRA = 1 };
typedef struct par_present_desc {
    int32_t scale_x, scale_y; /* 1..PAR_MAX_SCALE each; they may differ (pixel-aspect correction) */
    int32_t pitch;            /* bytes from one output row to the next: a multiple of 4, >= 4 * width * scale_x */
    int32_t order;            /* PAR_PRESENT_RGBA: bytes red, green, blue, alpha as par_color;
                                 PAR_PRESENT_BGRA: red and blue exchanged (an SDL RGB888 / ARGB8888 surface) */
} par_present_desc;           /* 16 bytes */

/* How par_upscale_device (par_raytracer.h; nothing in the reference) magnifies a frame or an index plane: by one of the
 * EPX-family pixel-art scalers, onto a surface as par_present_desc describes one. */
enum { PAR_UPSCALE_SCALE2X = 2, PAR_UPSCALE_SCALE3X = 3, PAR_UPSCALE_SCALE4X = 4 };   /* the value is the factor k */
typedef struct par_upscale_desc {
    int32_t scaler;  /* one of the three */
    int32_t pitch;   /* bytes between output rows of `out`: a multiple of 4, >= 4 * width * k (formed in 64 bits) */
    int32_t order;   /* PAR_PRESENT_RGBA or PAR_PRESENT_BGRA, as par_present_desc */
} par_upscale_desc;  /* 12 bytes */

/* The work block of the fitted-palette calls (par_palette_*_device, par_raytracer.h; nothing in the reference): a 15-bit
 * colour histogram, the table the cut makes of it and the sums the palette's entries are the means of. The cell of a
 * pixel p is (p.red >> 3) | (p.green >> 3) << 5 | (p.blue >> 3) << 10. */
#define PAR_PALETTE_CELLS 32768
typedef struct par_palette_work {
    uint32_t hist[PAR_PALETTE_CELLS];  /* pixels counted per cell, modulo 2^32 */
    uint64_t sums[PAR_MAX_PALETTE][4]; /* per entry: sum of red, green, blue, and the pixel count */
    uint8_t lut[PAR_PALETTE_CELLS];    /* cell -> entry */
    int32_t n_entries;                 /* entries the cut made, 0..256 */
    int32_t reserved[3];
} par_palette_work;                    /* 172 048 bytes; device memory, 8-byte aligned */

/* The work block of par_palette_refine_device (par_raytracer.h; nothing in the reference): the tallies from which a
 * round selects every entry's per-channel median by radix, the high four bits of a channel value first and the low four
 * among the pixels that share the chosen high four. The call initialises what it needs; between calls the content is
 * the library's. */
typedef struct par_palette_refine_work {
    uint32_t bins[PAR_MAX_PALETTE][3][16]; /* per entry and channel: pixels counted per nibble value of the stage */
    uint32_t rank[PAR_MAX_PALETTE][4];     /* per channel: the median's rank within its high nibble; [3]: the pixels n_k */
    uint32_t high[PAR_MAX_PALETTE];        /* the chosen high nibbles where a par_color's word has them: 0x00B0G0R0 */
} par_palette_refine_work;                 /* 54 272 bytes; device memory, 8-byte aligned */

/* `Ray`, alt:30-33 (20 bytes: fp32 inverse direction + short origin, 2 bytes tail padding). */
typedef struct par_ray {
    float inv_x, inv_y, inv_z;
    int16_t ox, oy, oz;
    int16_t pad_;
} par_ray;

/*
 * View / grid parameters. The reference hard-codes these as constexpr (alt:116-131) and literals
 * (alt:281 background, alt:702 ambient); here they are runtime values whose defaults reproduce the reference.
 * Grid dimensions are ceil(width/bin), ceil(height/bin), ceil(length/bin): identical to alt:120-122 whenever the view
 * is a multiple of the bin size (as 480x320x320 / 40 is).
 */
typedef struct par_params {
    int32_t width;      /* view_width  alt:117 (480) */
    int32_t height;     /* view_height alt:118 (320) */
    int32_t length;     /* view_length alt:119 (320) */
    int32_t bin_size;   /* single_bin_cubic_size alt:116 (40) */
    float ambient;      /* ambient_light alt:702 (0.25f); must lie in [0,1] */
    uint8_t background; /* gray level of uncovered pixels, alt:281 (255/2 = 127) */
    uint8_t reserved_[3];
    int32_t palette_size; /* entries of `palette` in use, spr:60-65 (4) */
    par_color palette[PAR_MAX_PALETTE];
} par_params;

#ifdef __cplusplus
}
#endif
#endif /* PAR_TYPES_H */
