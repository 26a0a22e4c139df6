// tileset_extend_spans_check.cpp — par_tileset_extend_spans (csrc/par_hostcall.h), the bytes of the tile storage that
// par_tileset_extend_host copies up and down: for each case the two copies are made between two heap blocks of exactly
// capacity * tile_bytes bytes, so a span that names a byte beyond the storage is the sanitiser's to find, and the result
// is compared with what the contract says: the stored tiles go up, the added tiles come down, and the caller's bytes
// from min(T_out, capacity) tiles on stay. Built without HIP and run by tests/test_tileset_extend_cpu.py; prints
// "<checks> checks, <failures> failures".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "par_hostcall.h"

namespace {

long checks = 0, failures = 0;

void check(bool ok, const char* what, uint64_t t_in, uint64_t t_out, uint64_t capacity) {
    checks++;
    if (ok) return;
    failures++;
    if (failures <= 20) {
        std::printf("FAILED %s: T_in %llu T_out %llu capacity %llu\n", what, (unsigned long long)t_in, (unsigned long long)t_out,
                    (unsigned long long)capacity);
    }
}

void run(uint64_t t_in, uint64_t t_out, uint64_t capacity, size_t tile_bytes) {
    const size_t bytes = (size_t)capacity * tile_bytes;
    // exact heap blocks (a vector of 0 bytes has no storage to overrun: every span must then be empty)
    std::vector<uint8_t> host(bytes, 0x11), device(bytes, 0x22);
    const par_tile_spans up = par_tileset_extend_spans(t_in, t_in, capacity, tile_bytes);
    check(up.download_bytes == 0, "nothing comes down of a set that did not grow", t_in, t_out, capacity);
    if (up.upload_bytes) std::memcpy(device.data(), host.data(), up.upload_bytes);
    const uint64_t stored = t_in < capacity ? t_in : capacity, kept = t_out < capacity ? t_out : capacity;
    check(up.upload_bytes == stored * tile_bytes, "the stored tiles go up", t_in, t_out, capacity);
    // the device adds its tiles
    for (size_t i = (size_t)stored * tile_bytes; i < (size_t)kept * tile_bytes; i++) device[i] = 0x33;
    const par_tile_spans down = par_tileset_extend_spans(t_in, t_out, capacity, tile_bytes);
    check(down.download_offset + down.download_bytes <= bytes, "the span lies in the storage", t_in, t_out, capacity);
    if (down.download_bytes) std::memcpy(host.data() + down.download_offset, device.data() + down.download_offset, down.download_bytes);
    bool ok = true;
    for (size_t i = 0; i < bytes; i++) {
        const uint8_t want = i < (size_t)stored * tile_bytes ? 0x11 : (i < (size_t)kept * tile_bytes ? 0x33 : 0x11);
        ok = ok && host[i] == want;
    }
    check(ok, "stored and later bytes are the caller's, the added tiles the device's", t_in, t_out, capacity);
}

}  // namespace

int main() {
    const uint64_t counts[] = {0, 1, 2, 7, 8, 9, 40, 0x7FFFFFFFull, 0xFFFFFFFFull};
    for (size_t tile_bytes : {(size_t)64, (size_t)128, (size_t)256}) {
        for (uint64_t capacity : {(uint64_t)0, (uint64_t)1, (uint64_t)8, (uint64_t)33}) {
            for (uint64_t t_in : counts) {
                for (uint64_t t_out : counts) {
                    if (t_out >= t_in) run(t_in, t_out, capacity, tile_bytes);
                }
            }
        }
    }
    // the largest set: 2^20 tiles of 256 bytes, full and overfull
    run((1u << 20) - 3, (1u << 20) + 5, 1u << 20, 256);
    run((1u << 20) + 5, (1u << 20) + 9, 1u << 20, 256);
    std::printf("%ld checks, %ld failures\n", checks, failures);
    return failures ? 1 : 0;
}
