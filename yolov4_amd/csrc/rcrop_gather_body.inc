// The body of the resized-crop gather kernels: one block's tile.  Included INSIDE a __global__ function (one wave of kTileX
// threads, grid (ceil(S / kTileX), ceil(S / kTileY), samples)) that names its arguments jobs, n, S, ws and defines
//   RC_GATHER_U8 0   rcrop_gather_kernel (resample.hip): also nm, dst, dsb, dsc, dsh, dsw.  blockIdx.z < n: the sample's own
//                    pixels, outside its paste rectangle; n + b (launched only when the batch has a paste): the partner's
//                    pixels at the same place, inside the rectangle.  A block without a pixel of its kind leaves at once.
//                    The normalised fp32 pixel goes to dst through the four strides.
//   RC_GATHER_U8 1   randaug_gather_u8_kernel (randaug.hip): also u8.  Every record counts as one without a partner and the
//                    pixel goes, as it is, to the uint8 batch u8[n][S][S][3] (S <= 4096).
// Text, not a function: as a device function called from both kernels the fp32 gather measured 4 % slower than its own body.
    const int pass = !RC_GATHER_U8 && blockIdx.z >= (unsigned)n ? 1 : 0;
    const int tx0 = blockIdx.x * kTileX, ty0 = blockIdx.y * kTileY, b = blockIdx.z - pass * n;
    const int tx1 = min(tx0 + kTileX, S), ty1 = min(ty0 + kTileY, S);
    const int ox = tx0 + threadIdx.x;
    const y4_rcrop_job self = jobs[b];
    int px0 = 0, px1 = 0, py0 = 0, py1 = 0;                   // the paste rectangle; empty without a partner
    if (!RC_GATHER_U8 && self.paste_from >= 0) { px0 = self.paste_x0; px1 = self.paste_x1; py0 = self.paste_y0; py1 = self.paste_y1; }
    // the tile's share of the rectangle
    const int ix0 = max(tx0, px0), ix1 = min(tx1, px1), iy0 = max(ty0, py0), iy1 = min(ty1, py1);
    const bool any_in = ix0 < ix1 && iy0 < iy1;
    const bool rows_in = any_in && iy0 == ty0 && iy1 == ty1;  // every row of the tile crosses the rectangle
    const bool all_in = rows_in && ix0 == tx0 && ix1 == tx1;
    const bool in_x = ox >= px0 && ox < px1;

    if (pass == 0 ? all_in : !any_in) return;                 // block-uniform
    const y4_rcrop_job jb = pass ? jobs[self.paste_from] : self;
    const int ksx = rc_ksize(jb.crop_w, jb.res_w), ksy = rc_ksize(jb.crop_h, jb.res_h);
    const int* __restrict__ tabx = ws + jb.ws_offset / 4;
    const int* __restrict__ taby = tabx + rc_axis_words(S, ksx);
    const int* __restrict__ ky = taby + 2ll * S;

    int ymin[kTileY], yn[kTileY];                             // block-uniform, statically indexed
    int ylo = INT_MAX, yhi = 0;
#pragma unroll
    for (int j = 0; j < kTileY; ++j) {
        ymin[j] = 0;
        yn[j] = 0;
        if (ty0 + j < S) {
            ymin[j] = taby[2 * (ty0 + j)];
            yn[j] = taby[2 * (ty0 + j) + 1];
            ylo = min(ylo, ymin[j]);
            yhi = max(yhi, ymin[j] + yn[j]);
        }
    }

    if (ox >= S || (pass ? !in_x : (in_x && rows_in))) return;    // (no barrier anywhere in this function)
    const int i = jb.flip ? S - 1 - ox : ox;                  // the window column this output column shows
    const int xmin = tabx[2 * i], xn = tabx[2 * i + 1];
    const int* __restrict__ kx = tabx + 2ll * S + (long long)i * ksx;
    const unsigned char* __restrict__ col =
        (const unsigned char*)jb.src + (long long)jb.crop_y * jb.src_pitch + 3ll * (jb.crop_x + xmin);

    int acc[kTileY][3];
#pragma unroll
    for (int j = 0; j < kTileY; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 1 << (kPrecBits - 1);

    for (int r = ylo; r < yhi; ++r) {                         // rows of the crop
        const unsigned char* __restrict__ p = col + (long long)r * jb.src_pitch;
        int h0 = 1 << (kPrecBits - 1), h1 = h0, h2 = h0;
        for (int t = 0; t < xn; ++t) {
            const int k = kx[t];
            h0 += (int)p[3 * t] * k;
            h1 += (int)p[3 * t + 1] * k;
            h2 += (int)p[3 * t + 2] * k;
        }
        h0 = rc_clip8(h0);                                    // Pillow stores the horizontal pass as uint8
        h1 = rc_clip8(h1);
        h2 = rc_clip8(h2);
#pragma unroll
        for (int j = 0; j < kTileY; ++j) {
            const int t = r - ymin[j];
            if ((unsigned)t < (unsigned)yn[j]) {
                const int k = ky[(long long)(ty0 + j) * ksy + t];
                acc[j][0] += h0 * k;
                acc[j][1] += h1 * k;
                acc[j][2] += h2 * k;
            }
        }
    }

#if RC_GATHER_U8
    unsigned char* __restrict__ o = u8 + 3ll * S * S * b + 3ll * ox;
#else
    float* __restrict__ o = dst + (long long)b * dsb + (long long)ox * dsw;
#endif
#pragma unroll
    for (int j = 0; j < kTileY; ++j) {
        const int oy = ty0 + j;
        if (oy >= S) break;
        const bool inside = in_x && oy >= py0 && oy < py1;
        if (inside != (pass == 1)) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {                         // c: output channel; memory channel 2 - c under swap_rb
            const int v = rc_clip8(jb.swap_rb ? acc[j][2 - c] : acc[j][c]);
#if RC_GATHER_U8
            o[3 * oy * S + c] = (unsigned char)v;
#else
            o[(long long)c * dsc + (long long)oy * dsh] = __fdiv_rn((float)v - nm.mean[c], nm.std[c]);
#endif
        }
    }
