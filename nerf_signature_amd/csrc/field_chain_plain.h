// A FRAGMENT of k_field_fwd / k_field_fwd_twin (csrc/field.hip), not a header: one evaluation of the MLP chain on the tile's first-layer operand `feat`, included once per
// evaluation with the destinations named by CHAIN_SIGMAS, CHAIN_RGBS, CHAIN_GEO and CHAIN_MASKS (pointers; the last three may be null).  Text for the reason
// field_chain_pipelined.h gives: k_field_fwd's instantiations keep their instruction streams, the clean twin is a second textual evaluation.
// Names the including scope must provide (all read, none declared here):
//   P, kTrace              the precision tag and whether layer inputs are traced (template parameters / constants)
//   lds, kHalf             the staged forward fragments and the hi -> lo distance
//   lane, h                the lane (0..63) and its half (lane >> 5)
//   feat[2]                the first layer's B operand (typename P::Op)
//   tile, s, sl, live      the tile index, this lane's row, the row clamped to M - 1 (for loads) and s < M
//   dirs, stride, trace    view directions [M,3], the plane / trace stride, the ActTrace (read only when kTrace)
//   F0, F1                 fragment offsets (fieldmlp.h; color_branch uses F2 .. F4 itself)
// Names it declares (wrap a second inclusion in a scope of its own): hid, b4, mask_s, so, mask_c, geo8, rgb, mrow.
// Macros the includer defines and undefines around the #include: CHAIN_SIGMAS, CHAIN_RGBS, CHAIN_GEO, CHAIN_MASKS (pointers; the last three may be null).
        f32x16 hid[2];
        typename P::Op b4[4];
        mfma_layer<P, 2, 2>(lds, kHalf, F0, lane, feat, hid);
        const uint32_t mask_s = relu_to_operand<P>(hid, b4);
        if (kTrace) store_rows64(trace.hs, stride, s, h, hid, [](float v, int) { return v > 0.0f ? v : 0.0f; });
        f32x16 so[1];
        mfma_layer<P, 1, 4>(lds, kHalf, F1, lane, b4, so);

        // rows 0..15 of the sigma head: register r (< 8) of half h is row_of_reg(h, r); row 0 is log-density
        const bool live = s < M;
        if (live && h == 0) CHAIN_SIGMAS[s] = expf(so[0][0]);  // trunc_exp forward (activation.py:9)
        if (CHAIN_GEO != nullptr && live) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int rho = row_of_reg(h, r);
                if (rho >= 1) CHAIN_GEO[15 * (size_t)s + rho - 1] = so[0][r];
            }
        }
        uint32_t mask_c[2] = {0u, 0u};
        if (CHAIN_RGBS != nullptr) {
            float geo8[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) geo8[r] = so[0][r];
            if (h == 0) geo8[0] = 1.0f;  // the slot of row 0 carries the padded constant input (weight column 31)
            float rgb[3];
            color_branch<P>(lds, lane, h, dirs[3 * (size_t)sl], dirs[3 * (size_t)sl + 1], dirs[3 * (size_t)sl + 2], geo8, mask_c, rgb,
                            kTrace ? &trace : nullptr, stride, s);
            if (live && h == 0) { CHAIN_RGBS[3 * (size_t)s] = rgb[0]; CHAIN_RGBS[3 * (size_t)s + 1] = rgb[1]; CHAIN_RGBS[3 * (size_t)s + 2] = rgb[2]; }
        }
        if (CHAIN_MASKS != nullptr) {
            uint32_t *mrow = CHAIN_MASKS + (size_t)tile * 192 + lane;
            mrow[0] = mask_s; mrow[64] = mask_c[0]; mrow[128] = mask_c[1];
        }
