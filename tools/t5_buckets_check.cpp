// Stand-alone host check of pd_t5_relative_buckets (prompt-diffusion_amd/csrc/t5_buckets.cpp): no GPU, no engine.  Meant for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/t5_buckets_check.cpp prompt-diffusion_amd/csrc/t5_buckets.cpp -o t5_buckets_check
// Walks every length 1 .. 512 at T5's settings (32 buckets, max distance 128) into an exactly sized buffer, checks the properties the formula
// promises (range, symmetry of the two halves, monotonicity, a shorter row being the middle of a longer one) and the refusals.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int pd_t5_relative_buckets(int32_t L, int32_t num_buckets, int32_t max_distance, int32_t* out);
void pd_set_error(const char*, ...) {}

int main() {
    const int NB = 32, MD = 128;
    std::vector<int32_t> full(2 * 512 - 1);
    if (pd_t5_relative_buckets(512, NB, MD, full.data())) { std::puts("L = 512 refused"); return 1; }
    for (int L = 1; L <= 512; ++L) {
        std::vector<int32_t> row(2 * L - 1);   // exactly sized: a write past the end is the sanitizer's to catch
        if (pd_t5_relative_buckets(L, NB, MD, row.data())) { std::printf("L = %d refused\n", L); return 1; }
        for (int i = 0; i < 2 * L - 1; ++i) {
            const int d = i - (L - 1);
            if (row[i] < 0 || row[i] >= NB) { std::printf("L %d d %d: bucket %d out of range\n", L, d, row[i]); return 1; }
            if (row[i] != full[511 + d]) { std::printf("L %d d %d: %d differs from the L = 512 row's %d\n", L, d, row[i], full[511 + d]); return 1; }
            if (d > 0 && row[i] != row[L - 1 - d] + NB / 2) { std::printf("L %d d %d: halves not symmetric\n", L, d); return 1; }
            if (d > 0 && i > L && row[i] < row[i - 1]) { std::printf("L %d d %d: not monotone\n", L, d); return 1; }
        }
    }
    if (full[511] != 0 || full[0] != NB / 2 - 1 || full[1022] != NB - 1 || full[511 + 7] != NB / 2 + 7 || full[511 + 8] != NB / 2 + 8) { std::puts("anchor values wrong"); return 1; }
    int32_t one = -1;
    if (!pd_t5_relative_buckets(0, NB, MD, &one) || !pd_t5_relative_buckets(4, NB, MD, nullptr) || !pd_t5_relative_buckets(4, 31, MD, &one) ||
        !pd_t5_relative_buckets(4, NB, 8, &one) || one != -1) { std::puts("a bad argument was accepted"); return 1; }
    std::puts("t5_buckets_check: ok");
    return 0;
}
