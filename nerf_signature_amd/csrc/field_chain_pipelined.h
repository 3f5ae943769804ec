// A FRAGMENT of field_fwd_pipelined (csrc/field.hip), not a header: one evaluation of the MLP chain on the tile's first-layer operand `feat` and its direction
// (dx, dy, dz), included once per evaluation with the outputs named by CHAIN_MASK (uint32_t[3]), CHAIN_SIGMA (float) and CHAIN_RGB (float[3]).  Text, not a function or a
// lambda: the launch without a twin must stay the instruction stream it was -- through either, the register allocation of k_field_fwd_train moved (164 -> 166 VGPRs; as a
// loop over two passes it spilled) -- and a second textual evaluation is what the clean twin adds.
// Names the including scope must provide (all read, none declared here):
//   P                      the precision tag (template parameter; only F16 instantiates field_fwd_pipelined today)
//   lds, kHalf             the staged forward fragments and the hi -> lo distance (fieldmlp.h: mfma_layer / load_frags)
//   lane, h                the lane (0..63) and its half (lane >> 5)
//   feat[2]                the first layer's B operand (typename P::Op); the twin overwrites feat[1].v[3] between its two inclusions
//   dx, dy, dz             the tile's view direction (floats, already past the input barrier)
//   F0 .. F4               fragment offsets (fieldmlp.h)
// Names it declares (wrap a second inclusion in a scope of its own): hid, b4, so, a0 .. a4, geo8, sh, cin, hm, pick, ux, uy, uz, mask_c.
// Macros the includer defines and undefines around the #include: CHAIN_MASK, CHAIN_SIGMA, CHAIN_RGB.
        f32x16 hid[2];
        typename P::Op b4[4];
        f32x16 so[1];
        if constexpr (P::kMfmaPerProduct == 1) {
            // fp16: every layer's weight fragments are fetched from LDS as ONE burst, issued in front of the vector work that precedes the layer
            // (the ReLU / packing of the layer before: ~260 cycles) -- fetched one by one, each right in front of its MFMA, a fragment's LDS
            // latency (~100 cycles) was paid 24 times per tile: half of a wave's cycles were spent parked on lgkmcnt (SQ_WAIT_ANY).
            f16x8 a0[4], a1[4];
            load_frags(lds, F0, lane, a0);
            load_frags(lds, F1, lane, a1);
            __builtin_amdgcn_sched_barrier(0);
            mfma_regs<2, 2>(a0, feat, hid);
            CHAIN_MASK[0] = relu_to_operand<P>(hid, b4);
            mfma_regs<1, 4>(a1, b4, so);
        } else {
            mfma_layer<P, 2, 2>(lds, kHalf, F0, lane, feat, hid);
            CHAIN_MASK[0] = relu_to_operand<P>(hid, b4);
            mfma_layer<P, 1, 4>(lds, kHalf, F1, lane, b4, so);
        }
        CHAIN_SIGMA = expf(so[0][0]);  // trunc_exp forward (activation.py:9); row 0 of the sigma head lives in lane half 0
        float geo8[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) geo8[r] = so[0][r];
        if (h == 0) geo8[0] = 1.0f;  // the slot of row 0 carries the padded constant input (weight column 31)
        if constexpr (P::kMfmaPerProduct == 1) {     // color_branch() with the fragment bursts in front of the vector work
            f16x8 a2[4], a3[8], a4[4];
            load_frags(lds, F2, lane, a2);
            load_frags(lds, F3, lane, a3);
            __builtin_amdgcn_sched_barrier(0);
            const float ux = (dx + 1.0f) / 2.0f, uy = (dy + 1.0f) / 2.0f, uz = (dz + 1.0f) / 2.0f;   // (network_wtmk_tcnn.py:114-115)
            float sh[16];
            sh16(ux * 2.0f - 1.0f, uy * 2.0f - 1.0f, uz * 2.0f - 1.0f, sh);
            typename P::Op cin[2];
            const uint32_t hm = 0u - (uint32_t)h;     // a bit select (v_bfi): written as `h ? sh[8 + j] : sh[j]` the compiler indexes a scratch copy of sh[]
            auto pick = [&](int j) { return __uint_as_float((__float_as_uint(sh[j]) & ~hm) | (__float_as_uint(sh[8 + j]) & hm)); };
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                P::put2(cin[0], j >> 1, pick(j), pick(j + 1));
                P::put2(cin[1], j >> 1, geo8[j], geo8[j + 1]);
            }
            mfma_regs<2, 2>(a2, cin, hid);
            load_frags(lds, F4, lane, a4);
            __builtin_amdgcn_sched_barrier(0);
            CHAIN_MASK[1] = relu_to_operand<P>(hid, b4);
            mfma_regs<2, 4>(a3, b4, hid);
            CHAIN_MASK[2] = relu_to_operand<P>(hid, b4);
            mfma_regs<1, 4>(a4, b4, so);
#pragma unroll
            for (int c = 0; c < 3; ++c) CHAIN_RGB[c] = 1.0f / (1.0f + expf(-so[0][c]));  // rows 0..2 live in lane half 0
        } else {
            uint32_t mask_c[2] = {0u, 0u};
            color_branch<P>(lds, lane, h, dx, dy, dz, geo8, mask_c, CHAIN_RGB);
            CHAIN_MASK[1] = mask_c[0];
            CHAIN_MASK[2] = mask_c[1];
        }
