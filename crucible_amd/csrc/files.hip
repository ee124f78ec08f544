// files.hip -- the image writers of include/crucible_hip.h (PPM P3 as the reference writes it, P6, PNG) and the 8-bit
// quantisation they share.  Host code only.
#include "../../include/crucible_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include <zlib.h>

static uint32_t display_byte(double c) {   // impl Display for Color, utils.rs:422-437: (255.0 * c.sqrt()) as u32
    double v = 255.0 * std::sqrt(c);
    if (!(v == v) || v <= 0.0) return 0;
    if (v >= 4294967295.0) return 4294967295u;
    return (uint32_t)v;
}

extern "C" {

int32_t cr_quantize_rgb8(const void* rgb, int32_t real_type, int64_t n_pixels, uint8_t* out) {
    if (!rgb || !out || n_pixels < 0 || (real_type != CR_REAL_F32 && real_type != CR_REAL_F64)) return CR_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n_pixels * 3; i++) {
        double v = real_type == CR_REAL_F64 ? ((const double*)rgb)[i] : (double)((const float*)rgb)[i];
        uint32_t b = display_byte(v);
        out[i] = (uint8_t)(b > 255u ? 255u : b);
    }
    return CR_OK;
}

int32_t cr_write_ppm(const char* path, const void* rgb, int32_t real_type, int32_t w, int32_t hgt) {
    if (!path || !rgb || w < 1 || hgt < 1 || (real_type != CR_REAL_F32 && real_type != CR_REAL_F64)) return CR_ERR_INVALID_ARG;
    FILE* f = fopen(path, "w");   // OpenOptions write+create+truncate, camera/mod.rs:275-279
    if (!f) return CR_ERR_IO;
    // The text of `writeln!(file, "{color}")` per pixel (camera/mod.rs:306-311, utils.rs:422-437), formatted into memory
    // rows at a time: 2 M fprintf calls per 1080p frame took 0.3 s, as long as the frame's render.
    struct Dec { char s[4]; uint8_t n; };
    static const std::vector<Dec> table = [] { std::vector<Dec> t(256); for (int v = 0; v < 256; v++) t[(size_t)v].n = (uint8_t)snprintf(t[(size_t)v].s, 4, "%d", v); return t; }();
    bool ok = fprintf(f, "P3\n%d %d\n255\n", w, hgt) > 0;   // camera/mod.rs:286
    const int64_t npix = (int64_t)w * hgt, chunk = 1 << 16;
    std::vector<char> buf((size_t)chunk * 36);   // three u32 of up to 10 digits, two blanks, a newline
    for (int64_t p0 = 0; ok && p0 < npix; p0 += chunk) {   // row-major, j outer
        char* o = buf.data();
        const int64_t p1 = std::min(npix, p0 + chunk);
        for (int64_t i = p0; i < p1; i++) {
            for (int k = 0; k < 3; k++) {
                const double c = real_type == CR_REAL_F64 ? ((const double*)rgb)[3 * i + k] : (double)((const float*)rgb)[3 * i + k];
                const uint32_t v = display_byte(c);
                if (v < 256u) { const Dec& d = table[v]; memcpy(o, d.s, 3); o += d.n; }
                else o += snprintf(o, 11, "%u", v);   // a channel above 1: not a Color the reference could hold, printed as `as u32` would
                *o++ = k == 2 ? '\n' : ' ';
            }
        }
        ok = fwrite(buf.data(), 1, (size_t)(o - buf.data()), f) == (size_t)(o - buf.data());
    }
    ok = (fclose(f) == 0) && ok;
    return ok ? CR_OK : CR_ERR_IO;
}

int32_t cr_write_ppm_binary(const char* path, const void* rgb, int32_t real_type, int32_t w, int32_t hgt) {
    if (!path || !rgb || w < 1 || hgt < 1 || (real_type != CR_REAL_F32 && real_type != CR_REAL_F64)) return CR_ERR_INVALID_ARG;
    std::vector<uint8_t> bytes((size_t)w * hgt * 3);
    if (cr_quantize_rgb8(rgb, real_type, (int64_t)w * hgt, bytes.data()) != CR_OK) return CR_ERR_INVALID_ARG;
    FILE* f = fopen(path, "wb");
    if (!f) return CR_ERR_IO;
    bool ok = fprintf(f, "P6\n%d %d\n255\n", w, hgt) > 0 && fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    ok = (fclose(f) == 0) && ok;
    return ok ? CR_OK : CR_ERR_IO;
}

int32_t cr_write_pfm(const char* path, const void* data, int32_t real_type, int32_t w, int32_t hgt, int32_t channels) {
    if (!path || !data || w < 1 || hgt < 1 || (channels != 1 && channels != 3) || (real_type != CR_REAL_F32 && real_type != CR_REAL_F64))
        return CR_ERR_INVALID_ARG;
    FILE* f = fopen(path, "wb");
    if (!f) return CR_ERR_IO;
    bool ok = fprintf(f, "%s\n%d %d\n-1.0\n", channels == 3 ? "PF" : "Pf", w, hgt) > 0;
    const size_t row = (size_t)w * (size_t)channels;
    std::vector<float> line(row);
    for (int32_t j = hgt - 1; ok && j >= 0; j--) {   // rows bottom to top
        if (real_type == CR_REAL_F64) { const double* s = (const double*)data + (size_t)j * row; for (size_t k = 0; k < row; k++) line[k] = (float)s[k]; }
        else memcpy(line.data(), (const float*)data + (size_t)j * row, row * sizeof(float));
        if (__BYTE_ORDER__ != __ORDER_LITTLE_ENDIAN__)
            for (size_t k = 0; k < row; k++) { uint32_t u; memcpy(&u, &line[k], 4); u = __builtin_bswap32(u); memcpy(&line[k], &u, 4); }
        ok = fwrite(line.data(), sizeof(float), row, f) == row;
    }
    ok = (fclose(f) == 0) && ok;
    return ok ? CR_OK : CR_ERR_IO;
}

int32_t cr_write_png(const char* path, const void* rgb, int32_t real_type, int32_t w, int32_t hgt) {
    if (!path || !rgb || w < 1 || hgt < 1 || (real_type != CR_REAL_F32 && real_type != CR_REAL_F64)) return CR_ERR_INVALID_ARG;
    const size_t row = (size_t)w * 3;
    std::vector<uint8_t> raw((row + 1) * hgt);   // filter byte 0 (None) + RGB8 per scanline
    {
        std::vector<uint8_t> bytes(row * hgt);
        if (cr_quantize_rgb8(rgb, real_type, (int64_t)w * hgt, bytes.data()) != CR_OK) return CR_ERR_INVALID_ARG;
        for (int32_t y = 0; y < hgt; y++) { raw[(row + 1) * y] = 0; memcpy(&raw[(row + 1) * y + 1], &bytes[row * y], row); }
    }
    uLongf zlen = compressBound((uLong)raw.size());
    std::vector<uint8_t> z(zlen);
    if (compress2(z.data(), &zlen, raw.data(), (uLong)raw.size(), 1) != Z_OK) return CR_ERR_IO;   // level 1: output speed matters, not size
    FILE* f = fopen(path, "wb");
    if (!f) return CR_ERR_IO;
    auto be32 = [](uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; };
    bool ok = true;
    auto chunk = [&](const char* type, const uint8_t* data, uint32_t len) {
        uint8_t hdr[8];
        be32(hdr, len); memcpy(hdr + 4, type, 4);
        uint32_t crc = (uint32_t)crc32(0L, (const Bytef*)type, 4);
        if (len) crc = (uint32_t)crc32(crc, data, len);
        uint8_t tail[4];
        be32(tail, crc);
        ok = ok && fwrite(hdr, 1, 8, f) == 8 && (len == 0 || fwrite(data, 1, len, f) == len) && fwrite(tail, 1, 4, f) == 4;
    };
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    ok = fwrite(sig, 1, 8, f) == 8;
    uint8_t ihdr[13];
    be32(ihdr, (uint32_t)w); be32(ihdr + 4, (uint32_t)hgt);
    ihdr[8] = 8; ihdr[9] = 2; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;   // 8-bit, colour type 2 (RGB), no interlace
    chunk("IHDR", ihdr, 13);
    chunk("IDAT", z.data(), (uint32_t)zlen);
    chunk("IEND", nullptr, 0);
    ok = (fclose(f) == 0) && ok;
    return ok ? CR_OK : CR_ERR_IO;
}

}   // extern "C"
