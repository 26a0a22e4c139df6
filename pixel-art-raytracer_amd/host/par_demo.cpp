// par_demo.cpp — headless counterpart of the reference's `main` loop (src/alternative.cpp:502-833) on the C ABI.
//
// Builds the reference's default graybox world (alt:517-599), plays a key script the way the reference's event
// loop applies keys (alt:641-681: arrows/PgUp/PgDn move entity 0 by 5, a k j u h o move the light by 5), renders
// every frame on the GPU through libpar_raytracer.so, optionally draws the debug line (alt:763-772) and writes the
// frames as binary PPM (P6) instead of presenting them through SDL (alt:774-788). Prints the per-frame time like
// alt:815-817.
//
//   par_demo [--keys RRRRUUUUhhhhjjPP] [--frames N] [--out DIR] [--gif FILE] [--debug-line] [--as-sdl] [--size W H L]
//            [--palette-levels K] [--dither S] [--outline S,C,D] [--scale SX[,SY]] [--finish] [--upscale K]
//            [--palette-fit N] [--palette-refine I] [--dither-pattern N[,S]] [--cells CW,CH] [--tileset TW,TH[,FLIPS]]
//            [--tileset-shared CAP] [--tileset-budget K] [--cells-fit S,K[,R]] [--vram MACHINE[,DIR]] [--vram-show [backdrop]] [--machine-fit]
//
// --gif writes the frames as one animated GIF89a (100 ms per frame like the reference's gif.gif); a frame's colours
// are palette entries times a brightness, at most a few hundred distinct values, so each frame gets an exact local
// colour table (frames with more than 256 colours fall back to a 3-3-2 bit table). --as-sdl shows the frame as the
// reference's window does: its SDL_PIXELFORMAT_RGB888 texture reads the struct's `red` byte as blue on little-endian
// machines (alt:613, 772: the debug line comes out blue).
//
// --palette-levels K (with --gif) quantises every frame of the GIF on the GPU (par_quantize_host) to the scene's own
// palette, par_palette_ramp(params, K): each sprite-palette entry at K brightness bands, then the background. That
// palette is every frame's local colour table and the index plane is written as it comes back; --dither S (0..255) adds
// the ordered dither. The PPM frames of --out stay unquantised.
//
// --palette-fit N (with --gif; N = 1..256) gives every frame of the GIF a palette of N entries fitted to that frame on
// the GPU by median cut (par_palette_fit_host) and quantises the frame to it (par_quantize_host): the fitted palette is
// the frame's local colour table, the index plane is written as it comes back, --dither S applies as with
// --palette-levels. It is refused together with --palette-levels or --finish. The PPM frames stay unquantised.
// --palette-refine I (with --palette-fit; I = 1..16) refines each frame's fitted palette by I k-medians rounds on the GPU
// (par_palette_refine_host) before the frame is quantised to it.
// --dither-pattern N[,S] (with --palette-levels or --palette-fit; N = 1..16 candidates a pixel, S = 0..256 the strength
// of the error fed back, 256 when left out) takes the GIF's index planes from par_quantize_pattern_host, pattern
// dithering, in place of par_quantize_host. It is refused together with --dither or --finish.
// --cells CW,CH (with --palette-fit N, N = 2..16; CW and CH each 8 or 16) quantises every frame of the GIF under colour
// cells (par_quantize_cells_host): a cell of CW x CH pixels may use any two colours of the frame's fitted (and refined)
// palette. The pairs of that palette (par_cells_pairs: N * (N - 1) / 2 sub-palettes of two entries) are the frame's local
// colour table and the index plane is written as it comes back; --dither S keeps its meaning. It is refused together
// with --dither-pattern or --finish.
// --cells-fit S,K[,R] (with --cells CW,CH and --palette-fit N, K <= N <= 256; S sub-palettes of K = 1..16 entries,
// S * K <= 256, R = 0..32 rounds, 0 when left out) fits every frame's table of sub-palettes on the GPU through the add-on
// (par_cells_fit_host of addons/include/par_cells_fit.h, the master the frame's fitted and refined palette) in place of
// the pairs, and quantises the frame under it: the table is the frame's local colour table. It prints one line a frame,
// `cells fit frame <i>: <S> x <K>, error <E0> -> <ER>`: the summed L1 error under the seed table and after the rounds.
// --tileset TW,TH[,FLIPS] (with --gif and --palette-levels, --palette-fit or --cells, wherever a frame of the GIF is an
// index plane; TW and TH each 8 or 16, FLIPS a mask 0..3 of the mirrors allowed, 0 when left out) counts the distinct
// tiles of every frame's index plane on the GPU (par_tileset_build_host with capacity 0, behind the quantise) and prints
// one line a frame, `tileset frame <i>: <T> tiles of <N> cells`: whether the frame fits a tile budget. It changes no
// byte of the GIF.
// --tileset-shared CAP (with --tileset; CAP = 0..1048576 tiles) also keeps ONE tile set of capacity CAP across the GIF's
// frames, the way a tile map's set or a sprite sheet is kept: every frame's index plane extends it
// (par_tileset_extend_host, the same tiles and flips), and after the frame's `tileset frame` line it prints
// `tileset shared frame <i>: <new> new, <T> tiles, capacity <CAP>`: the tiles the frame adds, its upload, and whether
// the animation fits the budget (T <= CAP; beyond it T is an upper bound). It changes no byte of the GIF either.
// --tileset-budget K (with --tileset; K = 1..1024 tiles) also reduces every frame's own tile set to at most K tiles: the
// frame's set and map are built (par_tileset_build_host with the capacity of its count), reduced through the add-on
// (par_tileset_reduce_host of addons/include/par_tileset_reduce.h, the palette the frame's colour table), and right after
// the frame's `tileset frame` line it prints `tileset budget frame <i>: <T> -> <K'> tiles, error <E>`: the tiles kept
// and the summed L1 error of the reduced picture. A frame of more than 4096 tiles is beyond the add-on and is reported
// as such. It changes no byte of the GIF either.
// --vram MACHINE[,DIR] (with --cells and --tileset 8,8[,FLIPS]; MACHINE one of nes, gbc, sms, megadrive, snes, gba) exports
// every frame's cells index plane the way that machine loads it, through the add-on of addons/include/par_vram.h: the
// plane taken modulo the sub-palette size K (what a tile stores; K is 2, or --cells-fit's, and at most the 4 or 16 colours
// of the machine's tiles), the tile set of that local plane (par_tileset_build_host, the mirrors of --tileset), the set
// packed into the machine's tile format (par_vram_encode_tiles_host) and the map with every cell's sub-palette into its
// map words (par_vram_encode_map_host over the cells' cell_out). After the frame's tileset lines it prints
// `vram frame <i>: <T> tiles (<Tflat> flat), <B> tile bytes, <M> map bytes, bad <b>`: the tiles of the local plane and of
// the flat one, the bytes of both exports, and the tiles and cells the machine cannot show as they are (a palette or tile
// number beyond its word, a mirror it lacks). With DIR it writes frame_<i>.chr, frame_<i>.map and, except for nes,
// frame_<i>.pal (the frame's table as the machine's colour words). It changes no byte of the GIF.
// --vram-show [backdrop] (with --vram) draws every frame's export the way the machine shows it, through the add-on of
// addons/include/par_screen.h: one par_screen_draw_host over the frame's tile bytes, map words and colour words (the nes
// has no colour words: its table goes in as RGBA8 entries, and the cells' cell_out as the attribute grid) on a screen the
// size of the frame at scroll 0; with `backdrop` every tile pixel of value 0 shows entry 0. After the `vram frame` line it
// prints `screen frame <i>: bad <b>, error <E>`: the map cells that name no tile of the export, and the summed L1 over red,
// green and blue between the shown picture and the cells frame (the table's entry of every index). With --vram's DIR it
// writes frame_<i>.ppm. Without it nothing the demo prints or writes changes.
// --vram-objects [LIMIT] (with --vram-show; LIMIT 1..128 objects a scanline, the machine's nominal figure of
// par_objects_machine_limits when left out) shows every later frame the way the machine would: frame 0 is the level, whose
// table, colour words, local tile set, map and cell_out are kept, and frame i >= 1 is objects over it, through the add-on of
// addons/include/par_objects.h. The frame is quantised under frame 0's table (par_quantize_cells_host) and taken to its
// local plane, which extends a copy of the kept set (par_tileset_extend_host), so that both maps share one numbering;
// par_objects_from_maps_host makes an object of every cell that differs; the extended set is encoded, frame 0's screen is
// drawn and the objects are drawn over it with the hardware's transparency (value 0 shows the level) under LIMIT. After the
// frame's `screen frame` line it prints `objects frame <i>: <n> objects, <new> new tiles, dropped <d>, error <E>`: the
// differing cells, the tiles the frame adds to the level's, the objects dropped over the scanlines, and the summed L1 over
// red, green and blue against frame i's cells frame under frame 0's table. With --vram's DIR it writes
// frame_<i>.obj.ppm and, for nes and gbc, frame_<i>.oam (par_objects_pack). Without it nothing the demo prints or writes
// changes.
// --machine-fit (with --cells-fit and --vram) fits the table through the add-on of addons/include/par_machine_fit.h
// (par_machine_fit_host) instead: under the colour depth of the machine's colour words (the nes, which has none, fits at
// RGBA8) and, with K of 2 or more, one backdrop entry shared by every sub-palette. In the place of the `cells fit` line it
// prints `machine fit frame <i>: <S> x <K>, error <E0> -> <ER>`. Without it nothing the demo prints or writes changes.
//
// --outline S,C,D draws every frame's outlines on the GPU (par_outline_host) from the frame's own G-buffer: silhouettes
// scaled by S / 256, creases by C / 256, a silhouette between two entities from a depth difference of D (128,320,4 is a
// dark line and a light top edge). The frame is outlined as soon as it is rendered: before the debug line, before
// --palette-levels quantises it and before it is written as PPM or GIF.
//
// --scale SX[,SY] (with --out; each 1..16, SY defaults to SX) writes the PPM frames at W * SX x H * SY: the frame as it
// stands when it is written (after the outline, the debug line and --as-sdl's exchange) put on a surface of that size on
// the GPU (par_present_host, nearest neighbour, tight pitch, RGBA order). GIFs stay at view size.
//
// --finish (with --out, and with --outline or --palette-levels or both) makes every frame's PPM the surface of ONE
// par_finish_host call in place of the separate host calls: the style of --outline, the ramp of --palette-levels and
// --dither, the scale of --scale (default 1), tight pitch, RGBA order. With a ramp the PPM shows the ramp's colours, and
// the frame of --gif is that call's index plane; without a ramp the frame of --gif is the outlined frame at scale 1.
// --debug-line and --as-sdl act between the stages and are refused together with it.
//
// --upscale K (with --out; K = 2, 3 or 4) writes the PPM frames at W * K x H * K through a pixel-art scaler, Scale2x,
// Scale3x or Scale4x: the frame as it stands when it is written, exactly where --scale acts, through one
// par_upscale_host call at tight pitch in RGBA order. It is refused together with --scale or --finish. GIFs stay at view
// size.
//
// Letters: R L U D P N = right, left, up, down, page-up, page-down; a k j u h o as in the reference. Frame 0 gets no
// key; frame k applies key k-1 (cycling when --frames exceeds the script).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <utility>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "par_cells.h"
#include "par_cells_fit.h"
#include "par_machine_fit.h"
#include "par_objects.h"
#include "par_raytracer.h"
#include "par_screen.h"
#include "par_tileset.h"
#include "par_tileset_extend.h"
#include "par_tileset_reduce.h"
#include "par_vram.h"

static void apply_key(char k, par_aabb& player, par_light& light) {
    switch (k) {
        case 'L': player.px -= 5; break;  // SDLK_LEFT  alt:643-645
        case 'R': player.px += 5; break;  // SDLK_RIGHT alt:646-648
        case 'U': player.pz += 5; break;  // SDLK_UP    alt:649-651
        case 'D': player.pz -= 5; break;  // SDLK_DOWN  alt:652-654
        case 'N': player.py -= 5; break;  // PAGEDOWN   alt:655-657
        case 'P': player.py += 5; break;  // PAGEUP     alt:658-660
        case 'a': light.z -= 5; break;    // alt:661-663
        case 'k': light.z += 5; break;    // alt:664-666
        case 'j': light.y -= 5; break;    // alt:667-669
        case 'u': light.y += 5; break;    // alt:670-672
        case 'h': light.x -= 5; break;    // alt:673-675
        case 'o': light.x += 5; break;    // alt:676-678
        default: break;
    }
}

static bool write_ppm(const std::string& path, const par_color* fb, int w, int h) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, "P6\n%d %d\n255\n", w, h);
    std::vector<unsigned char> row((size_t)w * 3);
    for (int y = 0; y < h; y++) {
        for (int x = 0; x < w; x++) {
            const par_color c = fb[(size_t)y * w + x];
            row[(size_t)x * 3 + 0] = c.red;
            row[(size_t)x * 3 + 1] = c.green;
            row[(size_t)x * 3 + 2] = c.blue;
        }
        std::fwrite(row.data(), 1, row.size(), f);
    }
    std::fclose(f);
    return true;
}

// ---- animated GIF89a writer (frame sink replacing the SDL present, alt:774-788) ---------------------------------
class GifWriter {
  public:
    bool open(const std::string& path, int w, int h) {
        f_ = std::fopen(path.c_str(), "wb");
        if (!f_) return false;
        w_ = w; h_ = h;
        std::fwrite("GIF89a", 1, 6, f_);
        put16(w); put16(h);
        std::fputc(0x70, f_);  // no global colour table, 8 bits of colour resolution
        std::fputc(0, f_);
        std::fputc(0, f_);
        const unsigned char loop[] = {0x21, 0xFF, 0x0B, 'N', 'E', 'T', 'S', 'C', 'A', 'P', 'E', '2', '.', '0', 3, 1, 0, 0, 0};
        std::fwrite(loop, 1, sizeof(loop), f_);
        return true;
    }
    void frame(const std::vector<unsigned char>& rgb, int delay_cs) {
        // exact local colour table when the frame has at most 256 colours
        std::map<uint32_t, int> index;
        std::vector<unsigned char> table;
        std::vector<unsigned char> pix((size_t)w_ * h_);
        bool exact = true;
        for (size_t i = 0; i < pix.size() && exact; i++) {
            const uint32_t c = (uint32_t)rgb[i * 3] | ((uint32_t)rgb[i * 3 + 1] << 8) | ((uint32_t)rgb[i * 3 + 2] << 16);
            auto it = index.find(c);
            if (it == index.end()) {
                if (index.size() == 256) { exact = false; break; }
                it = index.emplace(c, (int)index.size()).first;
                table.push_back(rgb[i * 3]); table.push_back(rgb[i * 3 + 1]); table.push_back(rgb[i * 3 + 2]);
            }
            pix[i] = (unsigned char)it->second;
        }
        if (!exact) {  // 3-3-2 bit quantisation
            table.clear();
            for (int c = 0; c < 256; c++) {
                table.push_back((unsigned char)(((c >> 5) & 7) * 255 / 7));
                table.push_back((unsigned char)(((c >> 2) & 7) * 255 / 7));
                table.push_back((unsigned char)((c & 3) * 255 / 3));
            }
            for (size_t i = 0; i < pix.size(); i++) {
                pix[i] = (unsigned char)(((rgb[i * 3] >> 5) << 5) | ((rgb[i * 3 + 1] >> 5) << 2) | (rgb[i * 3 + 2] >> 6));
            }
        }
        table.resize(256 * 3, 0);
        image(pix, table, delay_cs);
    }
    // an index plane over a fixed palette of at most 256 entries: the palette, padded to 256, is the local colour table
    void frame(const std::vector<unsigned char>& index, const std::vector<par_color>& palette, int delay_cs) {
        std::vector<unsigned char> table;
        for (const par_color& c : palette) { table.push_back(c.red); table.push_back(c.green); table.push_back(c.blue); }
        table.resize(256 * 3, 0);
        image(index, table, delay_cs);
    }
    void close() {
        if (f_) { std::fputc(0x3B, f_); std::fclose(f_); f_ = nullptr; }
    }

  private:
    void image(const std::vector<unsigned char>& pix, const std::vector<unsigned char>& table, int delay_cs) {
        const unsigned char gce[] = {0x21, 0xF9, 4, 0, (unsigned char)(delay_cs & 0xFF), (unsigned char)(delay_cs >> 8), 0, 0};
        std::fwrite(gce, 1, sizeof(gce), f_);
        std::fputc(0x2C, f_);
        put16(0); put16(0); put16(w_); put16(h_);
        std::fputc(0x87, f_);  // local colour table, 256 entries
        std::fwrite(table.data(), 1, table.size(), f_);
        lzw(pix);
    }
    void put16(int v) { std::fputc(v & 0xFF, f_); std::fputc((v >> 8) & 0xFF, f_); }
    void emit(unsigned code, int bits) {
        acc_ |= (uint64_t)code << nacc_;
        nacc_ += bits;
        while (nacc_ >= 8) {
            block_.push_back((unsigned char)(acc_ & 0xFF));
            acc_ >>= 8; nacc_ -= 8;
            if (block_.size() == 255) flush_block();
        }
    }
    void flush_block() {
        if (block_.empty()) return;
        std::fputc((int)block_.size(), f_);
        std::fwrite(block_.data(), 1, block_.size(), f_);
        block_.clear();
    }
    void lzw(const std::vector<unsigned char>& pix) {
        const int min_bits = 8, clear = 1 << min_bits, eoi = clear + 1;
        std::fputc(min_bits, f_);
        std::unordered_map<uint32_t, int> dict;
        int next = eoi + 1, bits = min_bits + 1;
        acc_ = 0; nacc_ = 0;
        emit(clear, bits);
        int prefix = pix[0];
        for (size_t i = 1; i < pix.size(); i++) {
            const uint32_t key = ((uint32_t)prefix << 8) | pix[i];
            auto it = dict.find(key);
            if (it != dict.end()) { prefix = it->second; continue; }
            emit(prefix, bits);
            if (next < 4096) {
                dict.emplace(key, next);
                if (next == (1 << bits)) bits++;  // the code just added needs one more bit from now on
                next++;
            } else {
                emit(clear, bits);
                dict.clear();
                next = eoi + 1;
                bits = min_bits + 1;
            }
            prefix = pix[i];
        }
        emit(prefix, bits);
        emit(eoi, bits);
        if (nacc_ > 0) { block_.push_back((unsigned char)(acc_ & 0xFF)); acc_ = 0; nacc_ = 0; }
        flush_block();
        std::fputc(0, f_);  // block terminator
    }
    FILE* f_ = nullptr;
    int w_ = 0, h_ = 0;
    uint64_t acc_ = 0;
    int nacc_ = 0;
    std::vector<unsigned char> block_;
};

int main(int argc, char** argv) {
    std::string keys = "RRRRUUUUhhhhjjPP", out_dir, gif_path;
    int frames = -1, W = 480, H = 320, L = 320, palette_levels = 0, dither = 0, palette_fit = 0, palette_refine = 0;
    bool debug_line = false, as_sdl = false, outline = false, finish = false, dither_given = false;
    int pattern_depth = 0, pattern_strength = 256;  // depth 0: no --dither-pattern
    int scale_x = 0, scale_y = 0;  // 0: no --scale
    int upscale = 0;               // 0: no --upscale
    int cell_w = 0, cell_h = 0;    // 0: no --cells
    int fit_sub = 0, fit_size = 0, fit_rounds = 0;  // fit_sub 0: no --cells-fit
    int tile_w = 0, tile_h = 0, tile_flips = 0;  // 0: no --tileset
    int shared_capacity = -1;                    // -1: no --tileset-shared
    int tile_budget = 0;                         // 0: no --tileset-budget
    int vram_machine = -1;                       // -1: no --vram
    std::string vram_name, vram_dir;
    int vram_show = -1;                          // -1: no --vram-show; else its backdrop
    bool machine_fit = false;                    // --machine-fit
    int vram_objects = -1;                       // -1: no --vram-objects; 0: the machine's line limit; else LIMIT
    par_outline_style outline_style{4, 256, 256};
    for (int i = 1; i < argc; i++) {
        if (!std::strcmp(argv[i], "--keys") && i + 1 < argc) keys = argv[++i];
        else if (!std::strcmp(argv[i], "--frames") && i + 1 < argc) frames = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--out") && i + 1 < argc) out_dir = argv[++i];
        else if (!std::strcmp(argv[i], "--gif") && i + 1 < argc) gif_path = argv[++i];
        else if (!std::strcmp(argv[i], "--debug-line")) debug_line = true;
        else if (!std::strcmp(argv[i], "--as-sdl")) as_sdl = true;
        else if (!std::strcmp(argv[i], "--finish")) finish = true;
        else if (!std::strcmp(argv[i], "--palette-levels") && i + 1 < argc) palette_levels = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--dither") && i + 1 < argc) { dither = std::atoi(argv[++i]); dither_given = true; }
        else if (!std::strcmp(argv[i], "--dither-pattern") && i + 1 < argc) {
            char tail = 0;
            const bool alone = std::sscanf(argv[++i], "%d%c", &pattern_depth, &tail) == 1;
            if ((!alone && std::sscanf(argv[i], "%d,%d%c", &pattern_depth, &pattern_strength, &tail) != 2) || pattern_depth < 1 ||
                pattern_depth > 16 || pattern_strength < 0 || pattern_strength > 256) {
                std::fprintf(stderr, "--dither-pattern wants N[,S], N 1..16 and S 0..256, got %s\n", argv[i]);
                return 2;
            }
        }
        else if (!std::strcmp(argv[i], "--cells") && i + 1 < argc) {
            char tail = 0;
            if (std::sscanf(argv[++i], "%d,%d%c", &cell_w, &cell_h, &tail) != 2 || (cell_w != 8 && cell_w != 16) ||
                (cell_h != 8 && cell_h != 16)) {
                std::fprintf(stderr, "--cells wants CW,CH, each 8 or 16, got %s\n", argv[i]);
                return 2;
            }
        }
        else if (!std::strcmp(argv[i], "--cells-fit") && i + 1 < argc) {
            char tail = 0;
            const bool two = std::sscanf(argv[++i], "%d,%d%c", &fit_sub, &fit_size, &tail) == 2;
            if ((!two && std::sscanf(argv[i], "%d,%d,%d%c", &fit_sub, &fit_size, &fit_rounds, &tail) != 3) || fit_sub < 1 ||
                fit_size < 1 || fit_size > PAR_CELLS_FIT_MAX_SUB_SIZE || fit_sub > PAR_MAX_PALETTE / fit_size || fit_rounds < 0 ||
                fit_rounds > PAR_CELLS_FIT_MAX_ROUNDS) {
                std::fprintf(stderr, "--cells-fit wants S,K[,R], K 1..%d, S * K at most %d and R 0..%d, got %s\n",
                             PAR_CELLS_FIT_MAX_SUB_SIZE, PAR_MAX_PALETTE, PAR_CELLS_FIT_MAX_ROUNDS, argv[i]);
                return 2;
            }
        }
        else if (!std::strcmp(argv[i], "--tileset") && i + 1 < argc) {
            char tail = 0;
            const bool two = std::sscanf(argv[++i], "%d,%d%c", &tile_w, &tile_h, &tail) == 2;
            if ((!two && std::sscanf(argv[i], "%d,%d,%d%c", &tile_w, &tile_h, &tile_flips, &tail) != 3) ||
                (tile_w != 8 && tile_w != 16) || (tile_h != 8 && tile_h != 16) || tile_flips < 0 || tile_flips > 3) {
                std::fprintf(stderr, "--tileset wants TW,TH[,FLIPS], TW and TH each 8 or 16 and FLIPS 0..3, got %s\n", argv[i]);
                return 2;
            }
        }
        else if (!std::strcmp(argv[i], "--tileset-shared") && i + 1 < argc) {
            char tail = 0;
            if (std::sscanf(argv[++i], "%d%c", &shared_capacity, &tail) != 1 || shared_capacity < 0 ||
                shared_capacity > PAR_TILESET_MAX_CELLS) {
                std::fprintf(stderr, "--tileset-shared wants a capacity of 0..%d tiles, got %s\n", PAR_TILESET_MAX_CELLS, argv[i]);
                return 2;
            }
        }
        else if (!std::strcmp(argv[i], "--tileset-budget") && i + 1 < argc) {
            char tail = 0;
            if (std::sscanf(argv[++i], "%d%c", &tile_budget, &tail) != 1 || tile_budget < 1 ||
                tile_budget > PAR_TILESET_REDUCE_MAX_BUDGET) {
                std::fprintf(stderr, "--tileset-budget wants 1..%d tiles, got %s\n", PAR_TILESET_REDUCE_MAX_BUDGET, argv[i]);
                return 2;
            }
        }
        else if (!std::strcmp(argv[i], "--vram") && i + 1 < argc) {
            static const char* const machines[] = {"nes", "gbc", "sms", "megadrive", "snes", "gba"};
            const std::string arg = argv[++i];
            const size_t comma = arg.find(',');
            vram_name = arg.substr(0, comma);
            if (comma != std::string::npos) vram_dir = arg.substr(comma + 1);
            for (int m = PAR_VRAM_NES; m <= PAR_VRAM_GBA; m++) {
                if (vram_name == machines[m]) vram_machine = m;
            }
            if (vram_machine < 0 || (comma != std::string::npos && vram_dir.empty())) {
                std::fprintf(stderr, "--vram wants MACHINE[,DIR], MACHINE one of nes, gbc, sms, megadrive, snes, gba, got %s\n", argv[i]);
                return 2;
            }
        }
        else if (!std::strcmp(argv[i], "--machine-fit")) machine_fit = true;
        else if (!std::strcmp(argv[i], "--vram-show")) {
            vram_show = 0;
            if (i + 1 < argc && !std::strcmp(argv[i + 1], "backdrop")) { vram_show = 1; i++; }
        }
        else if (!std::strcmp(argv[i], "--vram-objects")) {
            vram_objects = 0;
            char tail = 0;
            int limit = 0;
            if (i + 1 < argc && std::sscanf(argv[i + 1], "%d%c", &limit, &tail) == 1) {
                vram_objects = limit;
                if (vram_objects < 1 || vram_objects > PAR_OBJECTS_MAX_LINE) {
                    std::fprintf(stderr, "--vram-objects wants a LIMIT of 1..%d objects a scanline, got %s\n", PAR_OBJECTS_MAX_LINE, argv[i + 1]);
                    return 2;
                }
                i++;
            }
        }
        else if (!std::strcmp(argv[i], "--palette-fit") && i + 1 < argc) {
            char tail;
            if (std::sscanf(argv[++i], "%d%c", &palette_fit, &tail) != 1 || palette_fit < 1 || palette_fit > PAR_MAX_PALETTE) {
                std::fprintf(stderr, "--palette-fit wants 1..%d, got %s\n", PAR_MAX_PALETTE, argv[i]);
                return 2;
            }
        }
        else if (!std::strcmp(argv[i], "--palette-refine") && i + 1 < argc) {
            char tail;
            if (std::sscanf(argv[++i], "%d%c", &palette_refine, &tail) != 1 || palette_refine < 1 || palette_refine > 16) {
                std::fprintf(stderr, "--palette-refine wants 1..16, got %s\n", argv[i]);
                return 2;
            }
        }
        else if (!std::strcmp(argv[i], "--outline") && i + 1 < argc) {
            int s = 0, c = 0, d = 0;
            if (std::sscanf(argv[++i], "%d,%d,%d", &s, &c, &d) != 3) { std::fprintf(stderr, "--outline wants S,C,D, got %s\n", argv[i]); return 2; }
            outline_style = par_outline_style{d, s, c};
            outline = true;
        }
        else if (!std::strcmp(argv[i], "--scale") && i + 1 < argc) {
            char tail = 0;
            const int got = std::sscanf(argv[++i], "%d,%d%c", &scale_x, &scale_y, &tail);
            if (got == 1) scale_y = scale_x;
            if ((got != 1 && got != 2) || (got == 1 && std::strchr(argv[i], ',')) || scale_x < 1 || scale_x > PAR_MAX_SCALE ||
                scale_y < 1 || scale_y > PAR_MAX_SCALE) {
                std::fprintf(stderr, "--scale wants SX[,SY], each 1..%d, got %s\n", PAR_MAX_SCALE, argv[i]);
                return 2;
            }
        }
        else if (!std::strcmp(argv[i], "--upscale") && i + 1 < argc) {
            char tail = 0;
            if (std::sscanf(argv[++i], "%d%c", &upscale, &tail) != 1 || upscale < PAR_UPSCALE_SCALE2X || upscale > PAR_UPSCALE_SCALE4X) {
                std::fprintf(stderr, "--upscale wants 2, 3 or 4, got %s\n", argv[i]);
                return 2;
            }
        }
        else if (!std::strcmp(argv[i], "--size") && i + 3 < argc) { W = std::atoi(argv[++i]); H = std::atoi(argv[++i]); L = std::atoi(argv[++i]); }
        else { std::fprintf(stderr, "unknown argument %s\n", argv[i]); return 2; }
    }
    if (frames < 0) frames = (int)keys.size() + 1;
    if (upscale != 0) {
        if (out_dir.empty()) { std::fprintf(stderr, "--upscale wants --out\n"); return 2; }
        if (scale_x != 0 || finish) { std::fprintf(stderr, "--upscale cannot go with --scale or --finish\n"); return 2; }
    }
    if (palette_fit != 0 && (palette_levels != 0 || finish)) {
        std::fprintf(stderr, "--palette-fit cannot go with --palette-levels or --finish: a frame has one palette\n");
        return 2;
    }
    if (palette_refine != 0 && palette_fit == 0) {
        std::fprintf(stderr, "--palette-refine wants --palette-fit: it refines the fitted palette\n");
        return 2;
    }
    if (pattern_depth != 0) {
        if (palette_levels == 0 && palette_fit == 0) {
            std::fprintf(stderr, "--dither-pattern wants --palette-levels or --palette-fit: it dithers towards a palette\n");
            return 2;
        }
        if (dither_given || finish) {
            std::fprintf(stderr, "--dither-pattern cannot go with --dither or --finish: a frame has one dither\n");
            return 2;
        }
    }
    if (fit_sub != 0 && cell_w == 0) {
        std::fprintf(stderr, "--cells-fit wants --cells CW,CH: it fits the sub-palettes of those cells\n");
        return 2;
    }
    if (fit_sub != 0 && (palette_fit < fit_size || palette_fit > PAR_MAX_PALETTE)) {
        std::fprintf(stderr, "--cells-fit %d,%d wants --palette-fit %d..%d: the master its lists are taken from\n", fit_sub, fit_size,
                     fit_size, PAR_MAX_PALETTE);
        return 2;
    }
    if (cell_w != 0) {
        if (fit_sub == 0 && (palette_fit < 2 || palette_fit > 16)) {
            std::fprintf(stderr, "--cells wants --palette-fit 2..16: a cell uses two colours of the fitted palette\n");
            return 2;
        }
        if (pattern_depth != 0 || finish) {
            std::fprintf(stderr, "--cells cannot go with --dither-pattern or --finish: they know one flat palette\n");
            return 2;
        }
    }
    if (tile_w != 0 && (gif_path.empty() || (palette_levels == 0 && palette_fit == 0))) {
        std::fprintf(stderr, "--tileset wants --gif and --palette-levels, --palette-fit or --cells: it counts the tiles of an index plane\n");
        return 2;
    }
    if (shared_capacity >= 0 && tile_w == 0) {
        std::fprintf(stderr, "--tileset-shared wants --tileset TW,TH[,FLIPS]: it keeps the set of those tiles across the frames\n");
        return 2;
    }
    if (tile_budget != 0 && tile_w == 0) {
        std::fprintf(stderr, "--tileset-budget wants --tileset TW,TH[,FLIPS]: it reduces the set of those tiles\n");
        return 2;
    }
    // --vram: the machine's tile format, its colour words (-1: none, the NES has a fixed master palette) and its layout
    static const int vram_formats[] = {PAR_VRAM_2BPP_PLANAR, PAR_VRAM_2BPP_ROWS, PAR_VRAM_4BPP_ROW_PLANES,
                                       PAR_VRAM_4BPP_PACKED_HI, PAR_VRAM_4BPP_ROWS, PAR_VRAM_4BPP_PACKED_LO};
    static const int vram_colours[] = {-1, PAR_VRAM_BGR555, PAR_VRAM_BGR222, PAR_VRAM_BGR333_MD, PAR_VRAM_BGR555, PAR_VRAM_BGR555};
    const int vram_sub_size = fit_sub != 0 ? fit_size : 2;
    if (vram_machine >= 0) {
        if (cell_w == 0 || tile_w != 8 || tile_h != 8) {
            std::fprintf(stderr, "--vram wants --cells CW,CH and --tileset 8,8[,FLIPS]: it exports the 8 x 8 tiles of a cells index plane, "
                                 "a cell one or two tiles a side\n");
            return 2;
        }
        const int most = vram_machine <= PAR_VRAM_GBC ? 4 : 16;
        if (vram_sub_size > most) {
            std::fprintf(stderr, "--vram %s wants sub-palettes of at most %d entries, --cells-fit S,K has K = %d\n", vram_name.c_str(), most,
                         vram_sub_size);
            return 2;
        }
    }
    if (vram_show >= 0 && vram_machine < 0) { std::fprintf(stderr, "--vram-show wants --vram MACHINE[,DIR]: it draws that export\n"); return 2; }
    if (vram_objects >= 0 && vram_show < 0) {
        std::fprintf(stderr, "--vram-objects wants --vram-show: it draws the objects over that screen\n");
        return 2;
    }
    if (machine_fit && (fit_sub == 0 || vram_machine < 0)) {
        std::fprintf(stderr, "--machine-fit wants --cells-fit S,K[,R] and --vram MACHINE[,DIR]: it fits that table for that machine\n");
        return 2;
    }
    if (finish) {
        if (out_dir.empty()) { std::fprintf(stderr, "--finish wants --out\n"); return 2; }
        if (!outline && palette_levels == 0) { std::fprintf(stderr, "--finish wants --outline or --palette-levels: without both it is --scale\n"); return 2; }
        if (debug_line || as_sdl) { std::fprintf(stderr, "--finish cannot go with --debug-line or --as-sdl: they act between its stages\n"); return 2; }
        if (scale_x == 0) scale_x = scale_y = 1;
    }

    par_params params;
    par_default_params(&params);
    params.width = W; params.height = H; params.length = L;

    // scene, alt:517-599 + light alt:624-626
    const int n = par_scene_graybox(W, L, nullptr, 0);
    std::vector<par_aabb> aabbs((size_t)n);
    par_scene_graybox(W, L, aabbs.data(), n);
    par_sprite tile;
    par_sprite_tile_floor(&tile);
    par_light light{(int16_t)W, (int16_t)(H / 2), (int16_t)(L / 4), 10};

    par_context* ctx = nullptr;
    int rc = par_create(&params, 0, &ctx);
    if (rc != PAR_OK) { std::fprintf(stderr, "par_create: %s\n", par_status_string(rc)); return 1; }
    if ((rc = par_set_sprites(ctx, &tile, 1)) != PAR_OK || (rc = par_set_entities(ctx, aabbs.data(), nullptr, n)) != PAR_OK ||
        (rc = par_set_light(ctx, &light)) != PAR_OK) {
        std::fprintf(stderr, "scene upload: %s (%s)\n", par_status_string(rc), par_last_error(ctx));
        return 1;
    }

    std::vector<par_color> fb((size_t)W * H);
    std::vector<par_pixel> gbuf((size_t)W * H);
    std::vector<unsigned char> rgb((size_t)W * H * 3);
    std::vector<par_color> surface;  // --scale, --upscale: the frame as the PPM shows it
    std::vector<par_color> view;     // --finish with --gif, no ramp, a scale other than 1: the outlined frame at view size
    if (scale_x > 0 && !out_dir.empty()) surface.resize((size_t)W * scale_x * H * scale_y);
    if (upscale != 0) surface.resize((size_t)W * upscale * H * upscale);
    // --palette-levels: the GIF's frames are index planes over the scene's ramp
    std::vector<par_color> ramp;
    std::vector<unsigned char> index;
    if (palette_levels != 0 && (finish || !gif_path.empty())) {
        ramp.resize(PAR_MAX_PALETTE);
        const int n_ramp = par_palette_ramp(&params, palette_levels, ramp.data(), (int)ramp.size());
        if (n_ramp < 0) { std::fprintf(stderr, "--palette-levels %d: %s\n", palette_levels, par_status_string(-n_ramp)); return 2; }
        ramp.resize((size_t)n_ramp);
        index.resize((size_t)W * H);
    }
    // --palette-fit: the GIF's frames are index planes over a palette fitted to each frame
    std::vector<par_color> fitted, pairs;  // (pairs: --cells, the table of the fitted palette's pairs)
    if (palette_fit != 0 && !gif_path.empty()) {
        fitted.resize((size_t)palette_fit);
        index.resize((size_t)W * H);
    }
    // the index plane of the frame as it stands over `pal`: the ordered dither of --dither, or --dither-pattern's
    const auto quantise = [&](const std::vector<par_color>& pal) {
        if (pattern_depth != 0) {
            const int status = par_quantize_pattern_host(&params, 0, pal.data(), (int)pal.size(), pattern_depth, pattern_strength,
                                                         fb.data(), 0, H, nullptr, index.data());
            if (status != PAR_OK) std::fprintf(stderr, "par_quantize_pattern_host: %s\n", par_status_string(status));
            return status;
        }
        const int status = par_quantize_host(&params, 0, pal.data(), (int)pal.size(), dither, fb.data(), 0, H, nullptr, index.data());
        if (status != PAR_OK) std::fprintf(stderr, "par_quantize_host: %s\n", par_status_string(status));
        return status;
    };
    // --tileset-shared: the one set the frames extend, and its count
    std::vector<unsigned char> shared_tiles;
    int shared_count = 0;
    if (shared_capacity > 0) shared_tiles.resize((size_t)shared_capacity * (size_t)(tile_w * tile_h));
    // --tileset-budget: frame f's own set of `tiles` tiles built, reduced to the budget over `pal` and printed
    const auto reduce_tiles = [&](int f, int tiles, const std::vector<par_color>& pal) -> int {
        if (tiles > PAR_TILESET_REDUCE_MAX_TILES) {
            std::printf("tileset budget frame %d: %d tiles, more than the %d a reduce takes\n", f, tiles, PAR_TILESET_REDUCE_MAX_TILES);
            return (int)PAR_OK;
        }
        const int cells = ((W + tile_w - 1) / tile_w) * ((H + tile_h - 1) / tile_h);
        const size_t tile_bytes = (size_t)(tile_w * tile_h);
        std::vector<unsigned char> set((size_t)tiles * tile_bytes), kept((size_t)tile_budget * tile_bytes);
        std::vector<uint32_t> tile_map((size_t)cells);
        int built = 0, left = 0;
        uint64_t error = 0;
        int status = par_tileset_build_host(&params, 0, index.data(), 0, H, tile_w, tile_h, 0, tile_flips, set.data(), tiles,
                                            tile_map.data(), &built);
        if (status != PAR_OK) {
            std::fprintf(stderr, "par_tileset_build_host: %s\n", par_status_string(status));
            return status;
        }
        status = par_tileset_reduce_host(0, set.data(), built, tile_w, tile_h, tile_flips, tile_map.data(), cells,
                                         reinterpret_cast<const uint8_t*>(pal.data()), (int)pal.size(), tile_budget, kept.data(),
                                         tile_map.data(), nullptr, &left, &error);
        if (status != PAR_OK) {
            std::fprintf(stderr, "par_tileset_reduce_host: %s\n", par_status_string(status));
            return status;
        }
        std::printf("tileset budget frame %d: %d -> %d tiles, error %llu\n", f, built, left, (unsigned long long)error);
        return (int)PAR_OK;
    };
    // --vram: every cell's sub-palette (the cells call's cell_out), and the flat plane's tile count --tileset printed last
    std::vector<unsigned char> chosen;
    if (vram_machine >= 0) chosen.resize((size_t)((W + cell_w - 1) / cell_w) * (size_t)((H + cell_h - 1) / cell_h));
    int flat_tiles = 0;
    // --vram-objects: the level, frame 0's export as it was shown
    struct {
        std::vector<par_color> table;
        std::vector<unsigned char> colours, set, words, chosen;
        std::vector<uint32_t> tile_map;
        int tiles = 0;
    } level;
    const auto write_file = [&](int f, const char* ext, const std::vector<unsigned char>& bytes) {
        char name[64];
        std::snprintf(name, sizeof(name), "/frame_%03d.%s", f, ext);
        FILE* file = std::fopen((vram_dir + name).c_str(), "wb");
        const bool ok = file && std::fwrite(bytes.data(), 1, bytes.size(), file) == bytes.size();
        if (file) std::fclose(file);
        if (!ok) std::fprintf(stderr, "cannot write %s%s\n", vram_dir.c_str(), name);
        return ok;
    };
    // --vram: frame f's index plane over `table` (sub-palettes of vram_sub_size entries) exported, printed and written
    const auto export_vram = [&](int f, const std::vector<par_color>& table) -> int {
        if (vram_machine < 0) return (int)PAR_OK;
        const int gcx = (W + 7) / 8, gcy = (H + 7) / 8, cells = gcx * gcy, format = vram_formats[vram_machine];
        std::vector<unsigned char> local(index.size()), set((size_t)cells * 64);
        for (size_t i = 0; i < index.size(); i++) local[i] = (unsigned char)(index[i] % vram_sub_size);
        std::vector<uint32_t> tile_map((size_t)cells);
        int tiles = 0, bad_tiles = 0, bad_cells = 0;
        int status = par_tileset_build_host(&params, 0, local.data(), 0, H, 8, 8, 0, tile_flips, set.data(), cells, tile_map.data(),
                                            &tiles);
        if (status != PAR_OK) {
            std::fprintf(stderr, "par_tileset_build_host: %s\n", par_status_string(status));
            return status;
        }
        std::vector<unsigned char> chr((size_t)tiles * par_vram_tile_bytes(format, 8, 8));
        if ((status = par_vram_encode_tiles_host(0, set.data(), cells, tiles, 8, 8, format, chr.data(), &bad_tiles)) != PAR_OK) {
            std::fprintf(stderr, "par_vram_encode_tiles_host: %s\n", par_status_string(status));
            return status;
        }
        par_vram_map_layout layout;
        par_vram_map_layout_preset(vram_machine, &layout);
        std::vector<unsigned char> words((size_t)cells * (size_t)layout.word_bytes);
        if ((status = par_vram_encode_map_host(0, &layout, tile_map.data(), gcx, gcy, chosen.data(), cell_w / 8, cell_h / 8, words.data(),
                                               &bad_cells)) != PAR_OK) {
            std::fprintf(stderr, "par_vram_encode_map_host: %s\n", par_status_string(status));
            return status;
        }
        std::printf("vram frame %d: %d tiles (%d flat), %zu tile bytes, %zu map bytes, bad %d\n", f, tiles, flat_tiles, chr.size(),
                    words.size(), bad_tiles + bad_cells);
        std::vector<par_color> screen;
        if (vram_show >= 0) {
            // the machine's last step: the export drawn on a screen the size of the frame (par_screen.h's layout is
            // par_vram.h's field for field, and its formats have equal values)
            const int n_colors = (int)std::min<size_t>(table.size(), 256), colour_format = vram_colours[vram_machine];
            par_screen_desc d;
            std::memcpy(&d.layout, &layout, sizeof(d.layout));
            d.tile_w = d.tile_h = 8, d.tile_format = format, d.n_tiles = tiles;
            d.map_w = gcx, d.map_h = gcy, d.ratio_x = cell_w / 8, d.ratio_y = cell_h / 8;
            d.pal_format = colour_format >= 0 ? colour_format : (int)PAR_SCREEN_RGBA8, d.n_colors = n_colors, d.sub_size = vram_sub_size;
            d.backdrop = vram_show, d.width = W, d.height = H, d.scroll_x = d.scroll_y = 0;
            std::vector<unsigned char> colours(4 * (size_t)n_colors);
            if (colour_format >= 0) {
                colours.resize(par_vram_palette_words(reinterpret_cast<const uint8_t*>(table.data()), n_colors, colour_format, colours.data()));
            } else {
                std::memcpy(colours.data(), table.data(), colours.size());
            }
            screen.resize((size_t)W * H);
            int bad_shown = 0;
            // (the nes keeps a cell's palette in its attribute table, which the export leaves to the caller: cell_out is that grid)
            if ((status = par_screen_draw_host(0, &d, chr.data(), words.data(), vram_machine == PAR_VRAM_NES ? chosen.data() : nullptr,
                                               colours.data(), nullptr, reinterpret_cast<uint8_t*>(screen.data()), nullptr, &bad_shown)) != PAR_OK) {
                std::fprintf(stderr, "par_screen_draw_host: %s\n", par_status_string(status));
                return status;
            }
            unsigned long long error = 0;
            for (size_t i = 0; i < screen.size(); i++) {
                const par_color meant = table[index[i]], got = screen[i];
                error += (unsigned long long)(std::abs((int)got.red - (int)meant.red) + std::abs((int)got.green - (int)meant.green) +
                                              std::abs((int)got.blue - (int)meant.blue));
            }
            std::printf("screen frame %d: bad %d, error %llu\n", f, bad_shown, error);
            if (vram_objects >= 0 && f == 0) {
                level.table = table, level.colours = colours, level.words = words, level.chosen = chosen, level.tile_map = tile_map;
                level.set.assign(set.begin(), set.begin() + (size_t)tiles * 64), level.tiles = tiles;
            } else if (vram_objects >= 0) {
                // frame f as objects over the level: quantised under the level's table, numbered against the level's set
                const int n_sub = (int)level.table.size() / vram_sub_size, rx = cell_w / 8, ry = cell_h / 8, ccx = (W + cell_w - 1) / cell_w;
                std::vector<unsigned char> plane(index.size()), picked(chosen.size()), shared((size_t)2 * cells * 64);
                if ((status = par_quantize_cells_host(&params, 0, level.table.data(), n_sub, vram_sub_size, cell_w, cell_h, dither, fb.data(), 0, H,
                                                      nullptr, plane.data(), picked.data())) != PAR_OK) {
                    std::fprintf(stderr, "par_quantize_cells_host: %s\n", par_status_string(status));
                    return status;
                }
                std::vector<unsigned char> plane_local(plane.size());
                for (size_t i = 0; i < plane.size(); i++) plane_local[i] = (unsigned char)(plane[i] % vram_sub_size);
                std::copy(level.set.begin(), level.set.end(), shared.begin());
                std::vector<uint32_t> frame_map((size_t)cells);
                int count = level.tiles, first_new = 0;
                if ((status = par_tileset_extend_host(&params, 0, plane_local.data(), 0, H, 8, 8, 0, tile_flips, shared.data(), 2 * cells, &count,
                                                      frame_map.data(), &first_new)) != PAR_OK) {
                    std::fprintf(stderr, "par_tileset_extend_host: %s\n", par_status_string(status));
                    return status;
                }
                // a byte a tile cell: the sub-palette of the colour cell it lies in
                std::vector<unsigned char> cells_bg((size_t)cells), cells_now((size_t)cells);
                for (int c = 0; c < cells; c++) {
                    const size_t cc = (size_t)((c % gcx) / rx) + (size_t)((c / gcx) / ry) * (size_t)ccx;
                    cells_bg[(size_t)c] = level.chosen[cc], cells_now[(size_t)c] = picked[cc];
                }
                std::vector<par_object> objects((size_t)cells);
                int n_objects = 0, bad_objects = 0, dropped = 0, bad_set = 0, bad_level = 0, line_limit = vram_objects, most = 0;
                if (line_limit == 0) par_objects_machine_limits(vram_machine, &line_limit, &most);
                if ((status = par_objects_from_maps_host(0, level.tile_map.data(), cells_bg.data(), frame_map.data(), cells_now.data(), gcx, gcy, 8,
                                                         8, 0, 0, cells, objects.data(), &n_objects)) != PAR_OK) {
                    std::fprintf(stderr, "par_objects_from_maps_host: %s\n", par_status_string(status));
                    return status;
                }
                std::vector<unsigned char> chr_shared((size_t)count * par_vram_tile_bytes(format, 8, 8));
                if ((status = par_vram_encode_tiles_host(0, shared.data(), 2 * cells, count, 8, 8, format, chr_shared.data(), &bad_set)) != PAR_OK) {
                    std::fprintf(stderr, "par_vram_encode_tiles_host: %s\n", par_status_string(status));
                    return status;
                }
                par_screen_desc ld = d;
                ld.n_tiles = count;
                std::vector<par_color> over_level((size_t)W * H);
                if ((status = par_screen_draw_host(0, &ld, chr_shared.data(), level.words.data(),
                                                   vram_machine == PAR_VRAM_NES ? level.chosen.data() : nullptr, level.colours.data(), nullptr,
                                                   reinterpret_cast<uint8_t*>(over_level.data()), nullptr, &bad_level)) != PAR_OK) {
                    std::fprintf(stderr, "par_screen_draw_host: %s\n", par_status_string(status));
                    return status;
                }
                par_objects_desc od;
                od.tile_w = od.tile_h = 8, od.tile_format = format, od.n_tiles = count, od.n_objects = cells, od.line_limit = line_limit;
                od.pal_format = d.pal_format, od.n_colors = d.n_colors, od.sub_size = vram_sub_size, od.pal_base = 0;
                od.bg_sub_size = vram_sub_size, od.opaque = 0, od.width = W, od.height = H;
                if ((status = par_objects_draw_host(0, &od, chr_shared.data(), objects.data(), n_objects, level.colours.data(), nullptr,
                                                    reinterpret_cast<uint8_t*>(over_level.data()), nullptr, &bad_objects, &dropped)) != PAR_OK) {
                    std::fprintf(stderr, "par_objects_draw_host: %s\n", par_status_string(status));
                    return status;
                }
                unsigned long long off = 0;
                for (size_t i = 0; i < over_level.size(); i++) {
                    const par_color meant = level.table[plane[i]], got = over_level[i];
                    off += (unsigned long long)(std::abs((int)got.red - (int)meant.red) + std::abs((int)got.green - (int)meant.green) +
                                                std::abs((int)got.blue - (int)meant.blue));
                }
                std::printf("objects frame %d: %d objects, %d new tiles, dropped %d, error %llu\n", f, n_objects, count - first_new, dropped, off);
                if (!vram_dir.empty()) {
                    char name[64];
                    std::snprintf(name, sizeof(name), "/frame_%03d.obj.ppm", f);
                    if (!write_ppm(vram_dir + name, over_level.data(), W, H)) { std::fprintf(stderr, "cannot write %s%s\n", vram_dir.c_str(), name); return -1; }
                    if (vram_machine <= PAR_VRAM_GBC && n_objects > 0) {
                        std::vector<unsigned char> oam(4 * (size_t)n_objects);
                        int unfit = 0;
                        par_objects_pack(vram_machine == PAR_VRAM_NES ? PAR_OBJECTS_OAM_NES : PAR_OBJECTS_OAM_GB, objects.data(), n_objects, oam.data(), &unfit);
                        if (!write_file(f, "oam", oam)) return -1;
                    }
                }
            }
        }
        if (vram_dir.empty()) return (int)PAR_OK;
        if (!screen.empty()) {
            char name[64];
            std::snprintf(name, sizeof(name), "/frame_%03d.ppm", f);
            if (!write_ppm(vram_dir + name, screen.data(), W, H)) { std::fprintf(stderr, "cannot write %s%s\n", vram_dir.c_str(), name); return -1; }
        }
        if (!write_file(f, "chr", chr) || !write_file(f, "map", words)) return -1;  // (any status but PAR_OK ends the run)
        if (vram_colours[vram_machine] >= 0) {
            std::vector<unsigned char> colours(2 * table.size());
            colours.resize(par_vram_palette_words(reinterpret_cast<const uint8_t*>(table.data()), (int)table.size(),
                                                  vram_colours[vram_machine], colours.data()));
            if (!write_file(f, "pal", colours)) return -1;
        }
        return (int)PAR_OK;
    };
    // --tileset: the tiles of the index plane of frame f as it stands over `pal`, counted and printed
    const auto count_tiles = [&](int f, const std::vector<par_color>& pal) -> int {
        if (tile_w == 0) return PAR_OK;
        int tiles = 0;
        const int status = par_tileset_build_host(&params, 0, index.data(), 0, H, tile_w, tile_h, 0, tile_flips, nullptr, 0,
                                                  nullptr, &tiles);
        if (status != PAR_OK) {
            std::fprintf(stderr, "par_tileset_build_host: %s\n", par_status_string(status));
            return status;
        }
        std::printf("tileset frame %d: %d tiles of %d cells\n", f, tiles,
                    ((W + tile_w - 1) / tile_w) * ((H + tile_h - 1) / tile_h));
        flat_tiles = tiles;
        if (tile_budget != 0) {
            const int budget_status = reduce_tiles(f, tiles, pal);
            if (budget_status != PAR_OK) return budget_status;
        }
        if (shared_capacity < 0) return (int)PAR_OK;
        int first_new = 0;
        const int shared_status = par_tileset_extend_host(&params, 0, index.data(), 0, H, tile_w, tile_h, 0, tile_flips,
                                                          shared_capacity > 0 ? shared_tiles.data() : nullptr, shared_capacity,
                                                          &shared_count, nullptr, &first_new);
        if (shared_status != PAR_OK) {
            std::fprintf(stderr, "par_tileset_extend_host: %s\n", par_status_string(shared_status));
            return shared_status;
        }
        std::printf("tileset shared frame %d: %d new, %d tiles, capacity %d\n", f, shared_count - first_new, shared_count,
                    shared_capacity);
        return (int)PAR_OK;
    };
    GifWriter gif;
    if (!gif_path.empty() && !gif.open(gif_path, W, H)) { std::fprintf(stderr, "cannot write %s\n", gif_path.c_str()); return 1; }
    const int mouse_x = 0, mouse_y = 0;  // the reference's mouse position before any motion event (alt:133-134)
    for (int f = 0; f < frames; f++) {
        if (f > 0 && !keys.empty()) {
            apply_key(keys[(size_t)(f - 1) % keys.size()], aabbs[0], light);
            par_update_aabbs(ctx, &aabbs[0], 0, 1);
            par_set_light(ctx, &light);
        }
        const auto t0 = std::chrono::steady_clock::now();
        par_outputs o{fb.data(), gbuf.data(), nullptr, nullptr, nullptr};
        if ((rc = par_render(ctx, &o, 0)) != PAR_OK) {
            std::fprintf(stderr, "par_render: %s (%s)\n", par_status_string(rc), par_last_error(ctx));
            return 1;
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::printf("frame %d: %.3fms  player <%d, %d, %d>  light <%d, %d, %d>\n", f, ms, aabbs[0].px, aabbs[0].py,
                    aabbs[0].pz, light.x, light.y, light.z);  // alt:815-817 prints the frame time
        if (finish) {
            const par_outline_style* style = outline ? &outline_style : nullptr;
            const par_pixel* g = outline ? gbuf.data() : nullptr;
            const par_color* pal = ramp.empty() ? nullptr : ramp.data();
            const par_present_desc desc{scale_x, scale_y, 4 * W * scale_x, PAR_PRESENT_RGBA};
            if ((rc = par_finish_host(&params, 0, style, g, 0, H, pal, (int)ramp.size(), pal ? dither : 0, &desc, fb.data(), 0, H,
                                      surface.data(), pal ? index.data() : nullptr)) != PAR_OK) {
                std::fprintf(stderr, "par_finish_host: %s\n", par_status_string(rc));
                return rc == PAR_ERR_INVALID_ARG ? 2 : 1;
            }
            char name[64];
            std::snprintf(name, sizeof(name), "/frame_%03d.ppm", f);
            if (!write_ppm(out_dir + name, surface.data(), W * scale_x, H * scale_y)) { std::fprintf(stderr, "cannot write %s%s\n", out_dir.c_str(), name); return 1; }
            if (pal && !gif_path.empty()) {
                if (count_tiles(f, ramp) != PAR_OK) return 1;
                gif.frame(index, ramp, 10);
            } else if (!gif_path.empty()) {
                // the outlined frame at view size: the surface itself at scale 1, else one more call at scale 1
                const par_color* shown = surface.data();
                if (scale_x != 1 || scale_y != 1) {
                    const par_present_desc one{1, 1, 4 * W, PAR_PRESENT_RGBA};
                    view.resize(fb.size());
                    if ((rc = par_finish_host(&params, 0, style, g, 0, H, nullptr, 0, 0, &one, fb.data(), 0, H, view.data(), nullptr)) != PAR_OK) {
                        std::fprintf(stderr, "par_finish_host: %s\n", par_status_string(rc));
                        return 1;
                    }
                    shown = view.data();
                }
                for (size_t i = 0; i < fb.size(); i++) { rgb[i * 3] = shown[i].red; rgb[i * 3 + 1] = shown[i].green; rgb[i * 3 + 2] = shown[i].blue; }
                gif.frame(rgb, 10);
            }
            continue;
        }
        if (outline && (rc = par_outline_host(&params, 0, &outline_style, gbuf.data(), 0, H, fb.data(), 0, H, fb.data(), nullptr)) != PAR_OK) {
            std::fprintf(stderr, "par_outline_host: %s\n", par_status_string(rc));
            return rc == PAR_ERR_INVALID_ARG ? 2 : 1;
        }
        if (debug_line) par_debug_line(&params, &gbuf[(size_t)mouse_y * W + mouse_x], mouse_x, &light, fb.data());
        if (as_sdl) {
            for (auto& c : fb) std::swap(c.red, c.blue);
        }
        if (!out_dir.empty()) {
            char name[64];
            std::snprintf(name, sizeof(name), "/frame_%03d.ppm", f);
            const par_color* shown = fb.data();
            if (upscale != 0) {
                const par_upscale_desc desc{upscale, 4 * W * upscale, PAR_PRESENT_RGBA};
                if ((rc = par_upscale_host(&params, 0, &desc, fb.data(), nullptr, nullptr, 0, 0, H, 0, H, surface.data(), nullptr)) != PAR_OK) {
                    std::fprintf(stderr, "par_upscale_host: %s\n", par_status_string(rc));
                    return rc == PAR_ERR_INVALID_ARG ? 2 : 1;
                }
                shown = surface.data();
            } else if (!surface.empty()) {
                const par_present_desc desc{scale_x, scale_y, 4 * W * scale_x, PAR_PRESENT_RGBA};
                if ((rc = par_present_host(&params, 0, &desc, fb.data(), nullptr, nullptr, 0, 0, H, surface.data())) != PAR_OK) {
                    std::fprintf(stderr, "par_present_host: %s\n", par_status_string(rc));
                    return rc == PAR_ERR_INVALID_ARG ? 2 : 1;
                }
                shown = surface.data();
            }
            const int kx = upscale != 0 ? upscale : scale_x, ky = upscale != 0 ? upscale : scale_y;
            const int sw = surface.empty() ? W : W * kx, sh = surface.empty() ? H : H * ky;
            if (!write_ppm(out_dir + name, shown, sw, sh)) { std::fprintf(stderr, "cannot write %s%s\n", out_dir.c_str(), name); return 1; }
        }
        if (!fitted.empty()) {
            int made = 0;
            if ((rc = par_palette_fit_host(&params, 0, fb.data(), 0, H, palette_fit, fitted.data(), &made)) != PAR_OK) {
                std::fprintf(stderr, "par_palette_fit_host: %s\n", par_status_string(rc));
                return 1;
            }
            if (palette_refine != 0 &&
                (rc = par_palette_refine_host(&params, 0, fb.data(), 0, H, fitted.data(), palette_fit, palette_refine, nullptr)) != PAR_OK) {
                std::fprintf(stderr, "par_palette_refine_host: %s\n", par_status_string(rc));
                return 1;
            }
            if (fit_sub != 0) {
                // (pairs: here the fitted table)
                pairs.resize((size_t)fit_sub * fit_size);
                std::vector<uint64_t> errors((size_t)fit_rounds + 1);
                if (machine_fit) {
                    // the depth of the machine's colour words (their formats and the depths are equal in value)
                    const int depth = vram_colours[vram_machine] >= 0 ? vram_colours[vram_machine] : (int)PAR_MACHINE_RGBA8;
                    if ((rc = par_machine_fit_host(0, reinterpret_cast<const uint8_t*>(fb.data()), W, H, cell_w, cell_h,
                                                   reinterpret_cast<const uint8_t*>(fitted.data()), palette_fit, fit_sub, fit_size,
                                                   fit_rounds, depth, fit_size >= 2 ? 1 : 0, reinterpret_cast<uint8_t*>(pairs.data()),
                                                   nullptr, errors.data())) != PAR_OK) {
                        std::fprintf(stderr, "par_machine_fit_host: %s\n", par_status_string(rc));
                        return 1;
                    }
                } else if ((rc = par_cells_fit_host(0, reinterpret_cast<const uint8_t*>(fb.data()), W, H, cell_w, cell_h,
                                                    reinterpret_cast<const uint8_t*>(fitted.data()), palette_fit, fit_sub, fit_size,
                                                    fit_rounds, reinterpret_cast<uint8_t*>(pairs.data()), nullptr, errors.data())) != PAR_OK) {
                    std::fprintf(stderr, "par_cells_fit_host: %s\n", par_status_string(rc));
                    return 1;
                }
                std::printf("%s fit frame %d: %d x %d, error %llu -> %llu\n", machine_fit ? "machine" : "cells", f, fit_sub, fit_size,
                            (unsigned long long)errors[0], (unsigned long long)errors[(size_t)fit_rounds]);
                if ((rc = par_quantize_cells_host(&params, 0, pairs.data(), fit_sub, fit_size, cell_w, cell_h, dither, fb.data(), 0, H,
                                                  nullptr, index.data(), chosen.empty() ? nullptr : chosen.data())) != PAR_OK) {
                    std::fprintf(stderr, "par_quantize_cells_host: %s\n", par_status_string(rc));
                    return 1;
                }
                if (count_tiles(f, pairs) != PAR_OK || export_vram(f, pairs) != PAR_OK) return 1;
                gif.frame(index, pairs, 10);
            } else if (cell_w != 0) {
                pairs.resize((size_t)palette_fit * (palette_fit - 1));
                const int n_sub = par_cells_pairs(fitted.data(), palette_fit, pairs.data(), (int)pairs.size());
                if (n_sub < 0) { std::fprintf(stderr, "par_cells_pairs: %s\n", par_status_string(-n_sub)); return 1; }
                if ((rc = par_quantize_cells_host(&params, 0, pairs.data(), n_sub, 2, cell_w, cell_h, dither, fb.data(), 0, H,
                                                  nullptr, index.data(), chosen.empty() ? nullptr : chosen.data())) != PAR_OK) {
                    std::fprintf(stderr, "par_quantize_cells_host: %s\n", par_status_string(rc));
                    return 1;
                }
                if (count_tiles(f, pairs) != PAR_OK || export_vram(f, pairs) != PAR_OK) return 1;
                gif.frame(index, pairs, 10);
            } else {
                if (quantise(fitted) != PAR_OK || count_tiles(f, fitted) != PAR_OK) return 1;
                gif.frame(index, fitted, 10);
            }
        } else if (!ramp.empty()) {
            if (quantise(ramp) != PAR_OK || count_tiles(f, ramp) != PAR_OK) return 1;
            gif.frame(index, ramp, 10);
        } else if (!gif_path.empty()) {
            for (size_t i = 0; i < fb.size(); i++) { rgb[i * 3] = fb[i].red; rgb[i * 3 + 1] = fb[i].green; rgb[i * 3 + 2] = fb[i].blue; }
            gif.frame(rgb, 10);  // 100 ms per frame, as the reference's gif.gif
        }
    }
    gif.close();
    par_destroy(ctx);
    return 0;
}
