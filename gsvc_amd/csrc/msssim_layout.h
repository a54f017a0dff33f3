// gsvc_amd/csrc/msssim_layout.h — the five-scale pyramid of MS-SSIM as the host lays it out: the sides and tiles of every scale and
// where the pooled pictures and the tile sums sit in a workspace.  Shared by gsvc_msssim (metrics.hip) and the MS-SSIM loss
// (msssim_loss.hip), which appends its own regions behind the pooled pictures.
#pragma once
#include "common.h"
#include "ssim_tile.h"

namespace gsvc {

constexpr int MS_SCALES = 5;

struct MsLayout {
    int h[MS_SCALES], w[MS_SCALES], tx[MS_SCALES], ty[MS_SCALES];
    int64_t pyr[MS_SCALES];            // byte offset of scale s's pooled x pictures (s >= 1); y follows x
    int64_t partials;                  // byte offset of the partials
    int64_t part_off[MS_SCALES];       // first partial (in floats) of a scale
    int64_t bytes;
};

static MsLayout ms_layout(int32_t P, int32_t H, int32_t W)
{
    MsLayout L;
    int64_t at = 0, parts = 0;
    int h = H, w = W;
    for (int s = 0; s < MS_SCALES; s++) {
        L.h[s] = h;
        L.w[s] = w;
        L.tx[s] = (w - (ST_TAPS - 1) + ST_TILE - 1) / ST_TILE;
        L.ty[s] = (h - (ST_TAPS - 1) + ST_TILE - 1) / ST_TILE;
        L.pyr[s] = at;
        if (s > 0) at += (int64_t)align_up((uint64_t)2 * P * h * w * sizeof(float), 256);
        L.part_off[s] = parts;
        parts += (int64_t)P * L.tx[s] * L.ty[s];
        h = (h + 1) / 2;
        w = (w + 1) / 2;
    }
    L.partials = at;
    L.bytes = at + (int64_t)align_up((uint64_t)parts * sizeof(float), 256);
    return L;
}

static bool ms_shape_ok(int32_t P, int32_t H, int32_t W)
{
    return P >= 1 && P <= 65535 && H > 160 && W > 160 && H <= 32768 && W <= 32768;
}

}  // namespace gsvc
