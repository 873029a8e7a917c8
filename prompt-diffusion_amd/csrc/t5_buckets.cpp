// pdengine: T5's relative-position buckets on the host (pd_t5_relative_buckets, include/pdengine.h).  Kept free of HIP so that the function can
// be built into a stand-alone host program (tools/t5_buckets_check.cpp) as well as into the library.
#include <cmath>
#include <cstdint>

void pd_set_error(const char* fmt, ...);

// T5Attention._relative_position_bucket, bidirectional, for relative position d = key - query
static int t5_bucket(int d, int num_buckets, int max_distance) {
    int nb = num_buckets / 2, ret = d > 0 ? nb : 0;
    const int n = d < 0 ? -d : d;
    const int max_exact = nb / 2;
    if (n < max_exact) return ret + n;
    int v = max_exact + (int)(std::log((double)n / max_exact) / std::log((double)max_distance / max_exact) * (nb - max_exact));
    if (v > nb - 1) v = nb - 1;
    return ret + v;
}

extern "C" int pd_t5_relative_buckets(int32_t L, int32_t num_buckets, int32_t max_distance, int32_t* out) {
    if (L < 1 || !out || num_buckets < 4 || num_buckets % 2 || max_distance <= num_buckets / 4) { pd_set_error("pd_t5_relative_buckets: bad argument"); return 1; }
    for (int i = 0; i < 2 * L - 1; ++i) out[i] = t5_bucket(i - (L - 1), num_buckets, max_distance);
    return 0;
}
