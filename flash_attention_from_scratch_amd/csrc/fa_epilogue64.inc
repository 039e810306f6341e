// fa_epilogue64.inc -- the item epilogue of the persistent kernel (store_item: finish l, normalise, RNE to 16 bit, through the
// wave's LDS staging area, whole-row non-temporal stores); included by fa_fwd_kernel64.hpp inside walk(), whose locals it captures.
            // O of one item: finish l, normalise, RNE to 16 bit (final_softmax_normalization
            // softmax.cuh:107-128; forward_kernel.cuh:186-203), through this wave's 8-KB LDS staging
            // area one 32-row Q tile at a time so that the global stores are whole 256-B rows (16 B per
            // lane, 4 rows per wave-instruction).  Wave-private: no barrier.  The 16-B chunk index is
            // XORed with (row & 15) so the 8-B writes and the 16-B reads are bank-conflict free.
            // zero_behind: O is cleared for the next item as soon as its last register has been read (eight MFMAs on a zero
            // operand, which then run under the second tile's LDS round trip and row stores instead of behind the seam's
            // row max: -0.3 k cycles per item)
            auto store_item = [&](uint16_t *Oc, const int qb_c, const int ord, const bool zero_behind) {
                FA_JIT(false);
                asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");  // last P.V -> VALU reads of O
                char *stage_o = smem + 2 * TR::kStages * TILE + wave * TR::kStageBytes;
                constexpr int NRG = (HSUB ? 16 : 32) / RPP;   // row groups of four per pass through the staging area (eight waves: 16-row halves)
                // lane-derived indices recomputed here from a volatile v_mbcnt: values derived from
                // threadIdx at kernel entry would stay live (and get spilled) across the whole item loop
                int lane;
                asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
                const int r31 = lane & 31, hi = lane >> 5;
                const int rsub = lane / CPR, chunk = lane & (CPR - 1);
                // rows RPP i + rsub of a tile: one scalar base for the 32 rows, a 32-bit lane offset per store; all reads first
                // (the waits then count down), and the read address is one XOR per row group: row = RPP i + rsub, so
                // chunk ^ swz_of(row) = (chunk ^ rsub) ^ (RPP i & 15)
                static_assert(D == 128 && RPP == 4, "epilogue address split");
                const unsigned lane_off = (unsigned)rsub * (unsigned)ss * 2u + (unsigned)chunk * 16u;
                const unsigned rd0 = (unsigned)rsub * ROWB + ((unsigned)(chunk ^ rsub) << 4);
                s16x8 v[NRG];
                auto read_rows = [&]() {
#pragma unroll
                    for (int i = 0; i < NRG; ++i)
                        v[i] = *(const s16x8 *)(stage_o + RPP * i * ROWB + (rd0 ^ (((RPP * i) & 15u) << 4)));
                };
                auto store_rows = [&](int qt, int half = 0) {
                    const uint16_t *rows0 = Oc + ((int64_t)qb_c * TR::kBr + wave * TR::kRowsPerWave + qt * 32 + half * 16) * ss;
#pragma unroll
                    for (int i = 0; i < NRG; ++i) {
                        // non-temporal: O is written once and not read again by this kernel (+1.3...2.8 % at
                        // seq_len <= 1024, where the store-issue-bound epilogue is a visible share).
                        // asm: scalar row base + 32-bit lane offset (hipcc builds a 64-bit address per lane and store)
                        if constexpr (RAG) {  // rows beyond the sequence are not stored
                            if (qb_c * TR::kBr + wave * TR::kRowsPerWave + qt * 32 + RPP * i + rsub >= args.seq_len) continue;
                        }
                        // (the row group's offset goes into the lane offset, one v_add per store: eight scalar row bases
                        // instead cost 16 SGPRs that hipcc kept live -- spilled to VGPR lanes -- across the whole item)
                        // s_nop 1: a store of more than 64 bits reads its data registers for two more cycles, and hipcc --
                        // which does not see the instruction inside the asm -- may reuse v[i] for the very next vector
                        // instruction (it did, for the next store's address: tools/isa_lint64.py, finding STDATA)
                        // nt: O is written once and not read again (sc1 / sc0 sc1 write-through and the default policy measured
                        // 0 / 0 / -0.1 ... -3 %: profiles/r04/tune64_store_policy.txt)
                        asm volatile("global_store_dwordx4 %0, %1, %2 nt\n\ts_nop 1" ::"v"(lane_off + (unsigned)(RPP * i) * (unsigned)ss * 2u), "v"(v[i]), "s"(rows0));
                    }
                };
                // TUNE & 512 (tools/tune64.hip; profiles/r06/s512_floor.txt): the second tile is converted into REGISTERS under
                // the first tile's LDS round trip and row stores, and goes through the staging area behind them
                constexpr bool OVL = (TUNE & 512) != 0 && QT == 2;
                u32x2 w_def[OVL ? DTILES : 1][4];
                // LSE: this item's rows of lse (scalar: the item's batch*head from its ordinal)
                float *lse_rows = nullptr;
                if constexpr (LSE) {
                    int bh_l, qb_l;
                    coords_of(ord, bh_l, qb_l);
                    lse_rows = lse + (bh_l * lse_len + qb_c * TR::kBr + wave * TR::kRowsPerWave);
                }
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) {
                    const float l_row = pair_sum(rs[qt][0] + rs[qt][1]);
                    if constexpr (LSE) {
                        // ln sum_j exp(s_j / sqrt d) = (log2 l + m c) ln 2, from the reference the row ended with: -neg_msc = m c, the
                        // running max (lazy form, second pass) or the first tile's max less the guard's binades (speculative first pass).
                        // Row r31 of Q tile qt; both lane halves hold it.  A failed item's rows are rewritten by the second pass.
                        if (hi == 0) lse_rows[qt * 32 + r31] = (__builtin_amdgcn_logf(l_row) - neg_msc[qt]) * 0.693147180559945309f;
                    }
                    if constexpr (FAST) {
                        // every P of the row is <= l: below the limit nothing overflowed on the way (fp32 exp2, the
                        // 16-bit P, fp32 O); NaN fails the compare too.  A failed item is stored all the same (its
                        // rows are rewritten by the second pass).
                        constexpr float kLimit = spec_limit64<DT>();
                        if (__ballot(!(l_row < kLimit)) != 0 || item_bad) failed |= 1ull << (ord < 63 ? ord : 63);
                    }
                    if constexpr (SPEC && !FAST) {
                        // (scalar: one more item of the second pass, for fa_fwd_stats -- a whole item whose two halves are
                        // both redone counts once, with its first half)
                        if (qt == 0 && (!HALF || !(ord & 1) || !((todo >> (parent(ord) < 63 ? parent(ord) : 63)) & 1ull))) ++failed;
                    }
                    const float inv = 1.0f / l_row;
                    if constexpr (HSUB) {   // eight waves: the tile through the 4-KB staging area in two 16-row halves (converted twice)
                        char *wph = stage_o + (r31 & 15) * ROWB + hi * 8;
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
#pragma unroll
                            for (int t = 0; t < DTILES; ++t) {
                                asm volatile("" : "+a"(O[qt][t]));
#pragma unroll
                                for (int rq = 0; rq < 4; ++rq) {
                                    typedef float f32x2 __attribute__((ext_vector_type(2)));
                                    const f32x2 lo2 = f32x2{O[qt][t][4 * rq], O[qt][t][4 * rq + 1]} * inv;
                                    const f32x2 hi2 = f32x2{O[qt][t][4 * rq + 2], O[qt][t][4 * rq + 3]} * inv;
                                    u32x2 w;
                                    w[0] = E::pack2(lo2[0], lo2[1]);
                                    w[1] = E::pack2(hi2[0], hi2[1]);
                                    if ((r31 >> 4) == h) *(u32x2 *)(wph + (((4 * t + rq) ^ swz_of(r31)) << 4)) = w;
                                }
                                __builtin_amdgcn_sched_barrier(0);
                            }
                            if (h == 1 && zero_behind) zero_o();
                            read_rows();
                            store_rows(qt, h);
                        }
                        continue;
                    }
                    char *wp = stage_o + r31 * ROWB + hi * 8;
#pragma unroll
                    for (int t = 0; t < DTILES; ++t) {
                        // (the tile's accumulator copies start here: hipcc otherwise reads all 128 up front and spills)
                        asm volatile("" : "+a"(O[qt][t]));
                        // regs 4rq..4rq+3 : d = 32t + 8rq + 4hi + 0..3  -> chunk 4t + rq, half hi.  Converted in
                        // pairs (one v_cvt_pk per two values; a per-element convert costs three instructions per pair)
#pragma unroll
                        for (int rq = 0; rq < 4; ++rq) {
                            typedef float f32x2 __attribute__((ext_vector_type(2)));
                            const f32x2 lo2 = f32x2{O[qt][t][4 * rq], O[qt][t][4 * rq + 1]} * inv;  // v_pk_mul_f32
                            const f32x2 hi2 = f32x2{O[qt][t][4 * rq + 2], O[qt][t][4 * rq + 3]} * inv;
                            u32x2 w;
                            w[0] = E::pack2(lo2[0], lo2[1]);
                            w[1] = E::pack2(hi2[0], hi2[1]);
                            if (OVL && qt == 1) w_def[OVL ? t : 0][rq] = w;
                            else *(u32x2 *)(wp + (((4 * t + rq) ^ swz_of(r31)) << 4)) = w;
                        }
                        __builtin_amdgcn_sched_barrier(0);   // one d tile at a time: S(0) of the next item is live
                    }
                    if (OVL && qt == 1) {
                        store_rows(0);
#pragma unroll
                        for (int t = 0; t < DTILES; ++t)
#pragma unroll
                            for (int rq = 0; rq < 4; ++rq) *(u32x2 *)(wp + (((4 * t + rq) ^ swz_of(r31)) << 4)) = w_def[OVL ? t : 0][rq];
                    }
                    if (qt == QT - 1 && zero_behind) zero_o();
                    read_rows();
                    if (!(OVL && qt == 0)) store_rows(qt);
                }
            };
