// par_cells_fit.hip — the fitted-cells add-on (libpar_cells_fit.so): the table of per-cell sub-palettes fitted to a frame
// (par_cells_fit_device, par_cells_fit_host). The contract is beside the declarations in addons/include/par_cells_fit.h;
// nothing here knows a par_context or a par_params, and nothing here is linked into libpar_raytracer.so.
//
// The steps are par_cells_fit_steps.h's, which the machine-fit add-on shares: this unit is the order of the launches and the
// two entry points. The launches of a call, 4 + S + 4 * R, one more with errors_out: the entry, the cell pass, A_0, the S
// steps, per round the assign pass that tallies high nibbles, a select, the assign pass that tallies low nibbles and the
// select that moves the entries, then the emit and the assign pass for errors_out[R].
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "par_cells_fit.h"
#include "par_cells_fit_steps.h"
#include "par_hostcall.h"

namespace {

__global__ __launch_bounds__(CF_MAX_TABLE) void fit_emit_kernel(Fit w, uint32_t entries, uint8_t* table_out) {
    const uint32_t k = threadIdx.x;
    if (k >= entries) return;
    fit_emit(w, k, k, table_out);
}

template <int CW, int CH>
hipError_t launch_fit(hipStream_t stream, const FitCall& a) {
    const Geo g = geo_of<CW, CH>(a.width, a.height);
    const Fit w = fit_of(a.work, cells_of(a.width, a.height, CW, CH));
    const uint32_t* fb = reinterpret_cast<const uint32_t*>(a.fb);
    const uint32_t S = (uint32_t)a.n_sub, K = (uint32_t)a.sub_size;
    u64* errors = reinterpret_cast<u64*>(a.errors_out);
    const dim3 block(CF_THREADS), some(std::min(g.groups, CF_TALLY_GROUPS));

    hipError_t e = launch_lists<CW, CH>(stream, a, w, g, a.palette);
    if (e == hipSuccess) e = launch_steps<CW, CH>(stream, a, w, g, a.palette);
    for (int r = 0; r < a.rounds && e == hipSuccess; r++) {
        hipLaunchKernelGGL((fit_assign_kernel<CW, CH, CF_HI>), some, block, 0, stream, w, fb, g, a.n_sub, a.sub_size,
                           errors ? errors + r : nullptr);
        hipLaunchKernelGGL(fit_select_kernel<false>, dim3(1), dim3(CF_MAX_TABLE), 0, stream, w, S * K);
        hipLaunchKernelGGL((fit_assign_kernel<CW, CH, CF_LO>), some, block, 0, stream, w, fb, g, a.n_sub, a.sub_size, nullptr);
        hipLaunchKernelGGL(fit_select_kernel<true>, dim3(1), dim3(CF_MAX_TABLE), 0, stream, w, S * K);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fit_emit_kernel, dim3(1), dim3(CF_MAX_TABLE), 0, stream, w, S * K, a.table_out);
    if (errors) {
        hipLaunchKernelGGL((fit_assign_kernel<CW, CH, CF_ERROR>), dim3(std::min(g.groups, 4u * CF_TALLY_GROUPS)), block, 0, stream,
                           w, fb, g, a.n_sub, a.sub_size, errors + a.rounds);
    }
    return hipGetLastError();
}

hipError_t launch_fit(hipStream_t stream, int cell_w, int cell_h, const FitCall& a) {
    if (cell_w == 8) return cell_h == 8 ? launch_fit<8, 8>(stream, a) : launch_fit<8, 16>(stream, a);
    return cell_h == 8 ? launch_fit<16, 8>(stream, a) : launch_fit<16, 16>(stream, a);
}

}  // namespace

extern "C" {

size_t par_cells_fit_work_bytes(int width, int height, int cell_w, int cell_h) {
    const size_t cells = cells_of(width, height, cell_w, cell_h);
    return cells ? CF_HEAD_BYTES + CF_BYTES_PER_CELL * cells : 0;
}

int par_cells_fit_device(void* stream, const uint8_t* fb, int width, int height, int cell_w, int cell_h,
                         const uint8_t* palette, int n_colors, int n_sub, int sub_size, int rounds, void* work,
                         uint8_t* table_out, uint32_t* seeds_out, uint64_t* errors_out) {
    if (!fit_args_ok(fb, width, height, cell_w, cell_h, palette, n_colors, n_sub, sub_size, rounds, table_out) || !work ||
        (reinterpret_cast<uintptr_t>(work) & 7u) != 0) {
        return PAR_ERR_INVALID_ARG;
    }
    const FitCall a{fb, width, height, palette, n_colors, n_sub, sub_size, rounds, work, table_out, seeds_out, errors_out};
    return launch_fit((hipStream_t)stream, cell_w, cell_h, a) == hipSuccess ? PAR_OK : PAR_ERR_HIP;
}

int par_cells_fit_host(int device, const uint8_t* fb, int width, int height, int cell_w, int cell_h,
                       const uint8_t* palette, int n_colors, int n_sub, int sub_size, int rounds, uint8_t* table_out,
                       uint32_t* seeds_out, uint64_t* errors_out) {
    if (!fit_args_ok(fb, width, height, cell_w, cell_h, palette, n_colors, n_sub, sub_size, rounds, table_out)) {
        return PAR_ERR_INVALID_ARG;
    }
    const int rc = par_select_device(&device);
    if (rc != PAR_OK) return rc;
    hipError_t e = hipSetDevice(device);
    par_device_buffer d_fb(e, fb, (size_t)width * (size_t)height * 4, true);
    par_device_buffer d_palette(e, palette, (size_t)n_colors * 4, true);
    par_device_buffer d_work(e, fb, par_cells_fit_work_bytes(width, height, cell_w, cell_h), false);  // (device memory only)
    par_device_buffer d_table(e, table_out, (size_t)n_sub * (size_t)sub_size * 4, false);
    par_device_buffer d_seeds(e, seeds_out, (size_t)n_sub * sizeof(uint32_t), false);
    par_device_buffer d_errors(e, errors_out, (size_t)(rounds + 1) * sizeof(uint64_t), false);
    if (e == hipSuccess) {
        const FitCall a{d_fb.as<uint8_t>(), width, height, d_palette.as<uint8_t>(), n_colors, n_sub, sub_size, rounds,
                        d_work.as<void>(), d_table.as<uint8_t>(), d_seeds.as<uint32_t>(), d_errors.as<uint64_t>()};
        e = launch_fit(nullptr, cell_w, cell_h, a);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    d_table.download(table_out);
    if (seeds_out) d_seeds.download(seeds_out);
    if (errors_out) d_errors.download(errors_out);
    return par_status_of(e);
}

}  // extern "C"
