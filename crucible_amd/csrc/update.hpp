// In-place edits of an uploaded scene's primitives -- cr_update_primitives (include/crucible_hip.h).
//
// The caller hands over rows of 9 doubles with the meaning of CrPrimitive.v, named by their index in the description of
// the last upload.  The device keeps its primitive records in leaf order, so a per-scene table (descriptor index ->
// record position, -1 for a primitive without a record: hidden) takes each row to its record, and the row is converted
// exactly as pack_prim converts it on the host (pack.hpp): every coordinate rounded once to `real`, a sphere's 1/radius
// divided in `real`.  A sphere reads four values; what its record holds beyond them stays.  Kind, material and key range
// are not written.  The wrapper boxes are then re-derived by refit_level_kernel (refit.hpp) with use_keys = 0.
//
// cr_update_materials, cr_update_image add the two scatters below: a primitive's material index through the
// same table, and an image rectangle's RGB8 bytes into pack_images' texel words.  Both leave the tree alone.
#pragma once
#include "records.hpp"

namespace cr {

constexpr int kUpdateBlock = 256;

#if defined(__HIPCC__)
// One thread per row.  The block's rows are contiguous in `rows`: they are read with unit stride into LDS (a thread
// reading its own 72-byte row from global memory would touch nine cache lines' worth of strided words per wave
// instruction), and each thread then takes its row from there.  prim_index == nullptr: row r edits descriptor r.
template <typename real>
__global__ void __launch_bounds__(kUpdateBlock)
update_prims_kernel(Prim<real>* prims, int32_t n_records, const int32_t* desc_pos, int32_t n_desc, const int32_t* prim_index,
                    const double* rows, int32_t n) {
    __shared__ double tile[kUpdateBlock * 9];
    const int32_t base = (int32_t)blockIdx.x * kUpdateBlock;
    const int32_t here = n - base < kUpdateBlock ? n - base : kUpdateBlock;
    for (int32_t k = (int32_t)threadIdx.x; k < here * 9; k += kUpdateBlock) tile[k] = rows[(size_t)base * 9 + (size_t)k];
    __syncthreads();
    const int32_t r = base + (int32_t)threadIdx.x;
    if (r >= n) return;
    const int32_t desc = prim_index ? prim_index[r] : r;
    if (desc < 0 || desc >= n_desc) return;       // the host has validated the indices; nothing is written out of bounds regardless
    const int32_t pos = desc_pos[desc];
    if (pos < 0 || pos >= n_records) return;      // no device record (a hidden primitive): the host copy alone changes
    const double* v = tile + (int32_t)threadIdx.x * 9;
    Prim<real>& q = prims[pos];
    if (q.kind() == 0) {
        for (int k = 0; k < 4; k++) q.g[k] = (real)v[k];
        q.g[4] = real(1) / q.g[3];                // pack_prim's 1/radius
    } else {
        for (int k = 0; k < 9; k++) q.g[k] = (real)v[k];
    }
}

// cr_update_materials' assignment: one thread per (primitive, material) pair.  The record's kind stays and
// the material goes above it, as pack_prim writes kind_mat; nothing else of the record is touched.
template <typename real>
__global__ void __launch_bounds__(kUpdateBlock)
assign_materials_kernel(Prim<real>* prims, int32_t n_records, const int32_t* desc_pos, int32_t n_desc, const int32_t* prim_index,
                        const int32_t* prim_material, int32_t n) {
    const int32_t r = (int32_t)blockIdx.x * kUpdateBlock + (int32_t)threadIdx.x;
    if (r >= n) return;
    const int32_t desc = prim_index[r];
    if (desc < 0 || desc >= n_desc) return;       // the host has validated the indices; nothing is written out of bounds regardless
    const int32_t pos = desc_pos[desc];
    if (pos < 0 || pos >= n_records) return;      // no device record (a hidden primitive): the host copy alone changes
    Prim<real>& q = prims[pos];
    q.kind_mat = (q.kind_mat & 1) | (int32_t)((uint32_t)prim_material[r] << 1);
}

// cr_update_image: pack_images' texel word r | g << 8 | b << 16 (pack.hpp) for the texels of a width x height rectangle of an
// image_w-wide image whose first texel is texels[offset], from the staged RGB8 rows.  One thread per texel: a wave reads 192
// consecutive bytes and writes 64 consecutive words of one row (or of the rows the rectangle's width cuts them into).
__global__ void __launch_bounds__(kUpdateBlock)
pack_texels_kernel(uint32_t* texels, size_t n_texels, uint32_t offset, int32_t image_w, int32_t x0, int32_t y0, int32_t width, int32_t height,
                   const uint8_t* rgb8) {
    const size_t k = (size_t)blockIdx.x * kUpdateBlock + threadIdx.x;
    if (k >= (size_t)width * (size_t)height) return;
    const size_t j = k / (size_t)width, i = k - j * (size_t)width;
    const size_t dst = (size_t)offset + ((size_t)y0 + j) * (size_t)image_w + (size_t)x0 + i;
    if (dst >= n_texels) return;                  // the host has validated the rectangle; nothing is written out of bounds regardless
    const uint8_t* s = rgb8 + 3 * k;
    texels[dst] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
}
#endif

}   // namespace cr
