// The decision rules of the device-side SAH build (crucible_amd/csrc/sah_device.hpp: the CR_HD functions both of its
// phases call), compiled for the host with a plain C++ compiler and handed to tests/test_sah_device_host.py, which holds
// them to tests/sah_model.py.  `sah_device_check FILE`: FILE holds ranges, each a count m (u64) followed by m primitive
// boxes of six doubles (lo xyz, hi xyz) in the range's order.  Per range the program writes int32s to stdout: the axis
// and the plane sah_pick chooses (0 and -1 where nothing wins), the size of the left side, then every primitive's bin on
// the three axes.  The bins are gathered as the kernels gather them: centroid bounds and per-bin unions on sah_key's keys.
#include "sah_device.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace cr;

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: sah_device_check FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint64_t> w;
    uint64_t buf[4096];
    size_t got;
    while ((got = fread(buf, 8, 4096, f)) > 0) w.insert(w.end(), buf, buf + got);
    fclose(f);
    std::vector<int32_t> out;
    for (size_t at = 0; at < w.size();) {
        const uint64_t m = w[at++];
        if (m < 1 || m > (1u << 28) || at + 6 * m > w.size()) return 3;
        std::vector<double> box(6 * m);
        memcpy(box.data(), w.data() + at, 48 * m);
        at += 6 * m;
        uint64_t clo_k[3] = {kSahKeyPosInf, kSahKeyPosInf, kSahKeyPosInf}, chi_k[3] = {kSahKeyNegInf, kSahKeyNegInf, kSahKeyNegInf};
        for (uint64_t i = 0; i < m; i++) sah_bound_centroid(&box[6 * i], clo_k, chi_k);
        double clo[3], scale[3];
        bool ok[3];
        sah_axes(clo_k, chi_k, clo, scale, ok);
        SahBins* b = new SahBins;
        for (int j = 0; j < kSahAllBins; j++) b->cnt[j] = 0;
        for (int j = 0; j < kSahAllBins * 3; j++) { b->lo[j] = kSahKeyPosInf; b->hi[j] = kSahKeyNegInf; }
        std::vector<uint32_t> packed(m);
        for (uint64_t i = 0; i < m; i++) {
            const double* bx = &box[6 * i];
            packed[i] = sah_bins_of(bx, clo, scale, ok);
            for (int a = 0; a < 3; a++) {
                if (!ok[a]) continue;
                const int bin = a * kSahBins + (int)((packed[i] >> (4 * a)) & 15);
                b->cnt[bin]++;
                for (int d = 0; d < 3; d++) {
                    uint64_t l, h;
                    if (!sah_key(bx[d], l) || !sah_key(bx[3 + d], h)) continue;
                    if (l < b->lo[bin * 3 + d]) b->lo[bin * 3 + d] = l;
                    if (h > b->hi[bin * 3 + d]) b->hi[bin * 3 + d] = h;
                }
            }
        }
        uint32_t n_left = 0;
        const int win = sah_pick(*b, ok, n_left);
        delete b;
        out.push_back(win < kSahNone ? win / kSahPlanes : 0);
        out.push_back(win < kSahNone ? win % kSahPlanes : -1);
        out.push_back(win < kSahNone ? (int32_t)n_left : (int32_t)(m / 2));
        for (uint64_t i = 0; i < m; i++) for (int a = 0; a < 3; a++) out.push_back((int32_t)((packed[i] >> (4 * a)) & 15));
    }
    if (!out.empty() && fwrite(out.data(), 4, out.size(), stdout) != out.size()) return 4;
    return 0;
}
