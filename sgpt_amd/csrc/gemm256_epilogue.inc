// Epilogue of gemm256d_kernel (included inside the tile loop).  Expects in scope: EPI, OutT, SWAP, LO, p, out, acc[8][4], thv_pre[8],
// scr (this wave's 8-KiB LDS scratch), range (f16 range tracker), m0, n0, wm, wn, lane, fr, g.  Each wave round-trips its 128x64 sub-tile through LDS so that global stores are whole 128/256-byte rows.
        if constexpr (EPI == EPI_SCORE_FILTER) {
            // Scorer chunks after the first: the running k-th best score of query m is a lower bound of its final
            // k-th best, and a later document (higher index) never displaces an equal score, so only scores
            // STRICTLY above thr[m] can enter the top-k.  They are appended to the query's candidate list
            // (expected ~k per chunk under the doubling chunk schedule); nothing else leaves the registers.
            // MFMA C layout (SWAP): lane holds row m = fr of sub-tile i, columns 4g..4g+3 of sub-tile j.
            // Survivors are STAGED in this wave's 8-KiB LDS scratch and appended to the global lists in one flush per tile:
            //   * a row block whose lanes all fail the fast reject is skipped with one scalar branch;
            //   * in a block with survivors, each of the lane's 16 scores is tested with a wave-wide ballot: a slot nobody
            //     survives in costs a compare and a scalar branch; a slot with survivors gets its LDS positions from the
            //     ballot itself (base + mbcnt: no atomics), base being a wave-uniform scalar;
            //   * the flush hands ONE staged entry to each lane: the global atomics of a tile are all in flight together.
            // The per-lane form this replaces (NaN fix, count, atomicAdd, 16 predicated stores -- ~250 VALU instructions per
            // row block, executed by the whole wave as soon as ONE lane has a survivor, and one atomic round trip per block)
            // made a launch with ~0.4 survivors per row and tile (a 125 k-document shard filtered in one launch against sampled
            // thresholds) run at 541 TFLOP/s against ~1 000 without appends (profiles/r04_shard_profile.txt).
            // NaN scores count as -1 (exact_search.py:99): `v > th` is false for them, which is the right answer whenever
            // th >= -1 (cosine scores); a threshold below -1 (dot-product scores) takes the per-lane path below.
            if (has_tail && n0 == tail_n0) {      // the tile's columns >= tail_rows are copies of the last real document: never candidates
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            acc[i][j][r] = (wn * 64 + j * 16 + 4 * g + r) < tail_rows ? acc[i][j][r] : -INFINITY;
            }
            uint2_a* stage = reinterpret_cast<uint2_a*>(scr);             // [1024] x (row << 16 | column, score bits)
            int staged = 0;                                                // wave-uniform
            // this lane's (row, column) inside the wave's sub-tile; opaque to the optimiser, which otherwise hoists the 128
            // per-slot ids (lane-dependent, tile-invariant) out of the persistent tile loop: +128 live VGPRs, 400 spilled
            unsigned lane_id = ((unsigned)fr << 16) | (unsigned)(4 * g);
            asm volatile("" : "+v"(lane_id));
            // one threshold per row block (thv_pre: loaded by the tile loop under k-step 0); dot-product thresholds below -1
            // anywhere in the wave's rows -> general path
            float thv[8];
            bool neg = false;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                thv[i] = (m0 + wm * 128 + i * 16 + fr) < p.m_valid ? thv_pre[i] : INFINITY;     // padded query rows never append
                neg = neg || thv[i] < -1.0f;
            }
            if (__ballot(neg) != 0) {
                // the general per-lane path (NaN -> -1 can survive a threshold below -1)
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int m = m0 + wm * 128 + i * 16 + fr;
                    const float th = thv[i];
                    float mx = -INFINITY;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, acc[i][j][r]);
                    if ((mx > th || th < -1.0f) && cand_room(p.cand_cnt + m, p.cand_cap)) {
                        int c = 0;
#pragma unroll
                        for (int j = 0; j < 4; ++j)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float v = acc[i][j][r];
                                acc[i][j][r] = v != v ? -1.0f : v;       // cos_scores[isnan] = -1 (exact_search.py:99)
                                c += acc[i][j][r] > th ? 1 : 0;
                            }
                        int slot = atomicAdd(p.cand_cnt + m, c);
#pragma unroll
                        for (int j = 0; j < 4; ++j)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float v = acc[i][j][r];
                                if (v > th) {
                                    if (slot < p.cand_cap) {
                                        p.cand_val[(long)m * p.cand_cap + slot] = v;
                                        p.cand_idx[(long)m * p.cand_cap + slot] = p.idx_base + n0 + wn * 64 + j * 16 + 4 * g + r;
                                    }
                                    ++slot;
                                }
                            }
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float th = thv[i];
                    // Fast reject on the raw accumulators: fmaxf drops NaNs.  8 x v_max3 per row instead of 16 x (compare + select + max).
                    float mx = -INFINITY;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, acc[i][j][r]);
                    if (__ballot(mx > th) != 0) {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float v = acc[i][j][r];
                                const bool sv = v > th;
                                const unsigned long long mask = __ballot(sv);
                                if (mask != 0) {                                 // wave-uniform
                                    if (sv) {
                                        const int pos = staged + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                                        if (pos < 1024) stage[pos] = make_uint2(lane_id + (((unsigned)(i * 16) << 16) | (unsigned)(j * 16 + r)), __float_as_uint(v));
                                    }
                                    staged += __builtin_popcountll(mask);
                                }
                                __builtin_amdgcn_sched_barrier(0);               // one ballot live at a time (128 hoisted masks spill the SGPR file)
                            }
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
            if (staged > 0) {                                                // wave-uniform
                __builtin_amdgcn_wave_barrier();
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");           // the staged entries are in LDS (one wave: in order)
                // ONE global round trip per flush: the atomicAdd itself says whether the list still has room (a separate
                // capacity load in front of it was a second dependent round trip -- ~15 % of a tile's time at 24 entries per
                // wave and tile).  The storm case (every document beats the threshold) is bounded by the scratch instead: a
                // wave that staged more than it holds appends nothing and forces the chunk's fallback with one atomic.
                if (staged <= 1024) {
                    for (int e = lane; e < staged; e += 64) {
                        const uint2 ent = stage[e];
                        const int m = m0 + wm * 128 + (int)(ent.x >> 16);
                        const int slot = atomicAdd(p.cand_cnt + m, 1);
                        if (slot < p.cand_cap) {
                            p.cand_val[(long)m * p.cand_cap + slot] = __uint_as_float(ent.y);
                            p.cand_idx[(long)m * p.cand_cap + slot] = p.idx_base + n0 + wn * 64 + (int)(ent.x & 0xffffu);
                        }
                    }
                } else if (lane == 0) {
                    atomicAdd(p.cand_cnt + m0 + wm * 128 + (int)(stage[0].x >> 16), p.cand_cap + 1);   // raw > cap: cand_merge flags the chunk
                }
                __builtin_amdgcn_wave_barrier();
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
        } else if constexpr (EPI == EPI_SCORE_TOP2) {
            // The scorer's thresholds need a LOWER BOUND of every query's k-th best score that few documents beat; they used to be
            // the k-th best of a materialised score tile of a strided sample (31 MB for 1000 queries x 7 680 sampled documents,
            // written here and read back by a select launch: 32 + 23 us of a 0.28 ms shard pass).  The k-th best of any SUBSET of
            // the sample's scores is such a bound too: each wave keeps the two best of its 64 documents per query row -- with 120
            // (tile, wave) groups for 11 places the subset holds the sample's top-k but for the rare triple in one group -- and
            // only those 8 floats per row and tile leave the kernel.  NaN scores are skipped (they rank at -1, exact_search.py:99:
            // leaving a document out of a subset only lowers the bound).
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float m1 = -INFINITY, m2 = -INFINITY;
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v = acc[i][j][r];
                        v = v != v ? -INFINITY : v;
                        m2 = fmaxf(m2, fminf(m1, v));
                        m1 = fmaxf(m1, v);
                    }
#pragma unroll
                for (int sd = 16; sd <= 32; sd <<= 1) {          // the row's four lanes: fr, fr + 16, fr + 32, fr + 48
                    const float o1 = __shfl_xor(m1, sd, 64), o2 = __shfl_xor(m2, sd, 64);
                    m2 = fmaxf(fminf(m1, o1), fmaxf(m2, o2));
                    m1 = fmaxf(m1, o1);
                }
                const int m = m0 + wm * 128 + i * 16 + fr;
                if (g == 0 && m < p.m_valid)
                    *reinterpret_cast<float2*>(reinterpret_cast<float*>(out) + (long)m * p.ldo + (n0 >> 8) * 8 + wn * 2) = make_float2(m1, m2);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        } else if constexpr (EPI == EPI_NONE) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    asm volatile("" ::"v"(acc[i][j]));
                    acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
        } else if constexpr (SWAP && sizeof(OutT) == 2) {
            // bf16 row-major: 16 rows x 128 B per round, LDS row stride 144 B
            constexpr int RS = 144;
            const int rrow = lane >> 3, rchunk = lane & 7;
            float4 bb[4];
            const bool has_bias = epi_is_gelu(EPI) || p.bias != nullptr;   // plain store + bias: BLOOM Q/K projection
            // f16 range shifts (powers of two, 1 by default -- fma(acc, 1, b) == acc + b bit for bit):
            //   store: out = (acc * in_mul + bias) * out_mul = fma(acc, in_mul * out_mul, bias * out_mul)
            //   gelu : out = gelu(fma(acc, in_mul, bias)) * out_mul, the factor riding in the sigmoid's reciprocal
            // EPI_QKV: a V tile was computed with the operand roles swapped (see the tile loop): its rows are V features, its
            // columns tokens, its destination out2 = V^T
            OutT* e_out = out;
            long e_ldo = p.ldo;
            int e_m0 = m0, e_n0 = n0;
            float e_om = p.out_mul;
            if constexpr (EPI == EPI_QKV) {
                if (n0 >= p.n_split) { e_out = static_cast<OutT*>(p.out2); e_ldo = p.ldo2; e_m0 = n0 - p.n_split; e_n0 = m0; e_om = p.out_mul2; }
            }
            const float cs = epi_is_gelu(EPI) ? p.in_mul : p.in_mul * e_om;
            const float bsc = epi_is_gelu(EPI) ? 1.0f : e_om;
            const float ginv = 1.0f / e_om;
            if (has_bias) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    bb[j] = *reinterpret_cast<const float4*>(p.bias + e_n0 + wn * 64 + j * 16 + 4 * g);
                    bb[j].x *= bsc; bb[j].y *= bsc; bb[j].z *= bsc; bb[j].w *= bsc;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) bb[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            // running global pointer: rows advance by 8 per store instruction (no 64-bit multiply per store)
            char* gp = reinterpret_cast<char*>(e_out) + ((long)(e_m0 + wm * 128 + rrow) * e_ldo + e_n0 + wn * 64 + rchunk * 8) * 2;
            const long gstep = 16 * e_ldo;                                  // 8 rows x 2 bytes
#pragma unroll
            for (int i = 0; i < 8; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                    v[0] = __builtin_fmaf(v[0], cs, bb[j].x); v[1] = __builtin_fmaf(v[1], cs, bb[j].y);
                    v[2] = __builtin_fmaf(v[2], cs, bb[j].z); v[3] = __builtin_fmaf(v[3], cs, bb[j].w);
                    if constexpr (EPI == EPI_BIAS_GELU) {
                        v[0] = gelu_new_fast_scaled(v[0], ginv); v[1] = gelu_new_fast_scaled(v[1], ginv);
                        v[2] = gelu_new_fast_scaled(v[2], ginv); v[3] = gelu_new_fast_scaled(v[3], ginv);
                    }
                    if constexpr (EPI == EPI_BIAS_GELU_ERF) {
                        v[0] = gelu_erf(v[0]) * e_om; v[1] = gelu_erf(v[1]) * e_om;
                        v[2] = gelu_erf(v[2]) * e_om; v[3] = gelu_erf(v[3]) * e_om;
                    }
                    range.note(v[0], v[1]); range.note(v[2], v[3]);
                    const uint32_t h01 = Half<OutT>::pack2(v[0], v[1]), h23 = Half<OutT>::pack2(v[2], v[3]);
                    *reinterpret_cast<uint2_a*>(scr + fr * RS + (j * 16 + 4 * g) * 2) = make_uint2(h01, h23);
                    if constexpr (LO) {   // lo = round16(v - hi): the second half of the split-precision pair (second scratch tile)
                        *reinterpret_cast<uint2_a*>(scr + 16 * RS + fr * RS + (j * 16 + 4 * g) * 2) =
                            make_uint2(Half<OutT>::pack2(v[0] - Half<OutT>::lo(h01), v[1] - Half<OutT>::hi(h01)),
                                       Half<OutT>::pack2(v[2] - Half<OutT>::lo(h23), v[3] - Half<OutT>::hi(h23)));
                    }
                    acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int row = h * 8 + rrow;
                    const uint4 v = *reinterpret_cast<const uint4_a*>(scr + row * RS + rchunk * 16);
                    gstore16<true>(gp, v);
                    if constexpr (LO) {
                        const uint4 vl = *reinterpret_cast<const uint4_a*>(scr + 16 * RS + row * RS + rchunk * 16);
                        gstore16<true>(gp + 2 * p.lo_delta, vl);
                        if (p.hi2_delta != 0) gstore16<true>(gp + 2 * p.hi2_delta, v);
                    }
                    gp += gstep;
                }
            }
        } else if constexpr (SWAP) {
            // fp32 row-major (+bias +residual): 16 rows x 256 B per round, LDS row stride 272 B.
            // Each wave walks its 128x64 sub-tile in 8 rounds; the residual loads of a later round could be issued
            // before round i is processed.  Measured (scripts/gemm_bench.py): prefetch distance 0, 1, 2 -> 275 / 274 /
            // 273 us for the out-projection, and a start-up stagger of the workgroups changes nothing either: the
            // kernel's time is the SUM of its MFMA phase (115 us) and the read-modify-write of x at the rate a plain
            // streaming RMW kernel reaches (scripts/micro/rmw_bench.hip: 154 us, 5.2 TB/s) -- while the epilogues of
            // other CUs saturate HBM, the k-loops' operand DMA queues behind them and stalls (k-steps of 3.3-10 k
            // ticks instead of 2.7 k), so the two phases do not overlap however they are offset.
            constexpr int RS = 272;
            const int rrow = lane >> 4, rchunk = lane & 15;
            float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (EPI == EPI_BIAS_RESID) bb = *reinterpret_cast<const float4*>(p.bias + n0 + wn * 64 + rchunk * 4);
            // running element offset of this lane's 16-byte piece: 4 rows further per store (no 64-bit multiply per access)
            long goff = (long)(m0 + wm * 128 + rrow) * p.ldo + n0 + wn * 64 + rchunk * 4;
            const long gstep4 = 4 * p.ldo;
            // (Round 3 tried to start the accumulators as the residual tile -- MFMA C operand -- with the next tile's residual
            // fetched here, so that the epilogue would only add the bias and store: the 16-byte-per-lane C-layout loads were far
            // less efficient than these whole-row pieces and the launches got SLOWER: out-proj 236 -> 283 us, fc2 595 -> 700 us,
            // profiles/r03_resid_fold_ab.txt; the code is in the history.)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float4 rr[4];
                if constexpr (EPI == EPI_BIAS_RESID) {      // the round's four residual pieces, in flight during the LDS transpose
#pragma unroll
                    for (int h = 0; h < 4; ++h) rr[h] = ldg16<RESID_LD_NT>(p.resid + goff + h * gstep4);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    *reinterpret_cast<float4_a*>(scr + fr * RS + (j * 16 + 4 * g) * 4) =
                        make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
                    acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    float4 v = *reinterpret_cast<const float4_a*>(scr + (h * 4 + rrow) * RS + rchunk * 16);
                    if constexpr (EPI == EPI_BIAS_RESID) {   // acc * in_mul + (bias + resid); in_mul = 1: acc + (bias + resid) as before
                        v.x = __builtin_fmaf(v.x, p.in_mul, bb.x + rr[h].x); v.y = __builtin_fmaf(v.y, p.in_mul, bb.y + rr[h].y);
                        v.z = __builtin_fmaf(v.z, p.in_mul, bb.z + rr[h].z); v.w = __builtin_fmaf(v.w, p.in_mul, bb.w + rr[h].w);
                    }
                    bool keep = true;
                    if constexpr (EPI == EPI_SCORE) {   // cos_scores[isnan] = -1 (exact_search.py:99); padded query rows skipped
                        v.x = v.x != v.x ? -1.0f : v.x; v.y = v.y != v.y ? -1.0f : v.y;
                        v.z = v.z != v.z ? -1.0f : v.z; v.w = v.w != v.w ? -1.0f : v.w;
                        keep = m0 + wm * 128 + i * 16 + h * 4 + rrow < p.m_valid;
                    }
                    if (keep) gstore16<RESID_NT>(reinterpret_cast<float*>(out) + goff, __builtin_bit_cast(uint4, v));
                    goff += gstep4;
                }
            }
        } else {
            // V^T (bf16, out[n][m]): 16 n-rows x 256 B (128 m) per round, LDS row stride 272 B
            constexpr int RS = 272;
            const int rrow = lane >> 4, rchunk = lane & 15;
            char* gpt = reinterpret_cast<char*>(out) + ((long)(n0 + wn * 64 + rrow) * p.ldo + m0 + wm * 128 + rchunk * 8) * 2;
            const long gstept = 8 * p.ldo;                                  // 4 n-rows x 2 bytes
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float csv = p.in_mul * p.out_mul;                                  // f16 range shifts (1 by default)
                const float bn = (p.bias ? p.bias[n0 + wn * 64 + j * 16 + fr] : 0.f) * p.out_mul;   // BLOOM: V projection bias
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float v0 = __builtin_fmaf(acc[i][j][0], csv, bn), v1 = __builtin_fmaf(acc[i][j][1], csv, bn);
                    const float v2 = __builtin_fmaf(acc[i][j][2], csv, bn), v3 = __builtin_fmaf(acc[i][j][3], csv, bn);
                    range.note(v0, v1); range.note(v2, v3);
                    const uint32_t h01 = Half<OutT>::pack2(v0, v1), h23 = Half<OutT>::pack2(v2, v3);
                    *reinterpret_cast<uint2_a*>(scr + fr * RS + (i * 16 + 4 * g) * 2) = make_uint2(h01, h23);
                    if constexpr (LO) {   // the lo halves wait in the accumulator registers for the second pass through the scratch tile
                        acc[i][j] = f32x4{v0 - Half<OutT>::lo(h01), v1 - Half<OutT>::hi(h01), v2 - Half<OutT>::lo(h23), v3 - Half<OutT>::hi(h23)};
                    } else {
                        acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                }
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    const int row = h * 4 + rrow;
                    const uint4 v = *reinterpret_cast<const uint4_a*>(scr + row * RS + rchunk * 16);
                    gstore16<true>(gpt, v);
                    gpt += gstept;
                }
                if constexpr (LO) {       // (LDS operations of one wave execute in order: these writes queue behind the reads above)
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        *reinterpret_cast<uint2_a*>(scr + fr * RS + (i * 16 + 4 * g) * 2) =
                            make_uint2(Half<OutT>::pack2(acc[i][j][0], acc[i][j][1]), Half<OutT>::pack2(acc[i][j][2], acc[i][j][3]));
                        acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                    char* gl = gpt - 4 * gstept + 2 * p.lo_delta;
#pragma unroll
                    for (int h = 0; h < 4; ++h) {
                        const int row = h * 4 + rrow;
                        const uint4 v = *reinterpret_cast<const uint4_a*>(scr + row * RS + rchunk * 16);
                        gstore16<true>(gl, v);
                        gl += gstept;
                    }
                }
            }
        }
