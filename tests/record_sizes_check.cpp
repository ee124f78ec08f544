// record_sizes_check.cpp -- the bytes of the records a scene's LDS copy is made of (crucible_amd/csrc/records.hpp), as a
// plain C++ compiler sees them, and launch_plan.hpp's slot sizes at the block the residency comparisons budget for:
// one "name f64 f32" line each (tests/test_lds_capacity_host.py holds tests/lds_capacity.py to them).  queue.hpp's
// queue_state_bytes needs the HIP headers and is restated in the helper instead.
#include "launch_plan.hpp"
#include "records.hpp"

#include <cstdio>

int main() {
    using namespace cr;
    printf("entry %zu %zu\n", sizeof(Entry<double>), sizeof(Entry<float>));
    printf("entry_o %zu %zu\n", sizeof(EntryO<double>), sizeof(EntryO<float>));
    printf("screen %zu %zu\n", sizeof(ScreenEntry), sizeof(ScreenEntry));
    printf("screen_o %zu %zu\n", sizeof(ScreenEntryO), sizeof(ScreenEntryO));
    printf("prim %zu %zu\n", sizeof(Prim<double>), sizeof(Prim<float>));
    printf("mat %zu %zu\n", sizeof(Mat<double>), sizeof(Mat<float>));
    printf("tex %zu %zu\n", sizeof(Tex<double>), sizeof(Tex<float>));
    printf("max_block %d %d\n", MaxBlock<double>::value, MaxBlock<float>::value);
    for (int tile = 4; tile <= 6; tile++) printf("fx_lds_%d %zu %zu\n", tile, fx_lds_bytes(MaxBlock<double>::value, (uint32_t)tile), fx_lds_bytes(MaxBlock<float>::value, (uint32_t)tile));
    printf("aov_lds %zu %zu\n", aov_lds_bytes(MaxBlock<double>::value), aov_lds_bytes(MaxBlock<float>::value));
    return 0;
}
