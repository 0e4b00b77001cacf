// Where a bulk sgpt_encode call may be cut into two chains of whole sequences (encode.hip: encode_impl).  Plain C++, no HIP: the host
// program tests/encode_split_dump.cpp builds it with the host compiler (tests/test_encode_split.py).
#pragma once
#include <cstdint>

constexpr int ENCODE_SPLIT_TILE = 256;     // row tile of the 256x256 projection kernel: both chains start on one

// Chain A owns token rows [0, row) = sequences [0, seq), chain B the rest (the filler rows behind the last sequence included).
// row == 0: the call is not cut.
struct EncodeSplit { int32_t row, seq; };

// seq_off: HOST int32[B + 1], the sequence starts of the packed layout (include/sgpt_hip.h: sgpt_encode); T: its token rows.
// The cut is the sequence start nearest T / 2 that is a multiple of ENCODE_SPLIT_TILE rows and lies in the middle third of the
// call, [T / 3, 2 T / 3] (a cut further out leaves one chain the other cannot hide behind); the lower of two equally near ones.
// Both chains hold at least one sequence.  A layout that is not ascending, or runs past T, is not cut.
inline EncodeSplit encode_split_point(const int32_t* seq_off, int32_t B, int32_t T) {
    EncodeSplit best{0, 0};
    if (!seq_off || B < 2 || T <= 0 || seq_off[0] != 0) return best;
    int64_t best_dist = -1;
    for (int32_t b = 1; b <= B; ++b)
        if (seq_off[b] <= seq_off[b - 1] || seq_off[b] > T) return EncodeSplit{0, 0};
    for (int32_t b = 1; b < B; ++b) {
        const int64_t o = seq_off[b];
        if (o % ENCODE_SPLIT_TILE != 0 || 3 * o < T || 3 * o > 2 * (int64_t)T) continue;
        const int64_t dist = 2 * o > T ? 2 * o - T : T - 2 * o;
        if (best_dist < 0 || dist < best_dist) { best_dist = dist; best = EncodeSplit{(int32_t)o, b}; }
    }
    return best;
}
