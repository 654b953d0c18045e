// Per-pixel arithmetic of the photometric augmentation (augment.hip): PIL's ImageEnhance blends, its RGB <-> HSV conversions and one tap row of scipy's
// symmetric correlate1d, restated operation by operation so that the bytes are PIL's / scipy's. Plain C++ (host and device): every rounding below is part of the
// contract -- float32 where PIL's C computes in float, double where a double literal promotes the expression -- and nothing may be contracted into an FMA.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/pinmem_hip.h"

#ifdef __HIPCC__
#define PM_AUG_HD __host__ __device__ __forceinline__
#else
#define PM_AUG_HD static inline
#endif

#pragma clang fp contract(off)

enum { PM_AUG_BRIGHTNESS = 0, PM_AUG_CONTRAST = 1, PM_AUG_SATURATION = 2, PM_AUG_HUE = 3 };      // torchvision's fn_idx values
#define PM_AUG_MAX_RADIUS 5

// Image.blend(degenerate d, image v, alpha f) (libImaging/Blend.c): truncation inside [0, 1], clipping outside
PM_AUG_HD int pm_aug_blend(int d, int v, float f) {
  const float t = (float)d + f * (float)(v - d);
  if (f >= 0.f && f <= 1.f) return (int)t;
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}
// convert("L") (libImaging/Convert.c L24 >> 16)
PM_AUG_HD int pm_aug_grey(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }
PM_AUG_HD int pm_aug_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// convert("HSV") of one pixel (Convert.c rgb2hsv_row): h is a float, the literals 2.0 / 4.0 / 6.0 / 255.0 make their expressions double
PM_AUG_HD void pm_aug_rgb2hsv(int r, int g, int b, int* H8, int* S8) {
  const int mx = r > g ? (r > b ? r : b) : (g > b ? g : b), mn = r < g ? (r < b ? r : b) : (g < b ? g : b);
  *H8 = 0, *S8 = 0;
  if (mx == mn) return;
  const float cr = (float)(mx - mn);
  const float s = cr / (float)mx;
  const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
  float h;
  if (r == mx) h = bc - gc;
  else if (g == mx) h = (float)(2.0 + (double)rc - (double)bc);
  else h = (float)(4.0 + (double)gc - (double)rc);
  h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
  *H8 = pm_aug_clip8((int)((double)h * 255.0));
  *S8 = pm_aug_clip8((int)((double)s * 255.0));
}
// HSV -> RGB of one pixel (Convert.c hsv2rgb)
PM_AUG_HD void pm_aug_hsv2rgb(int H8, int S8, int V, int* r, int* g, int* b) {
  if (S8 == 0) {
    *r = *g = *b = V;
    return;
  }
  const float h = (float)H8 * 6.f / 255.f;
  const float fi = floorf(h);
  const int i = (int)fi;
  const float f = h - fi;
  const float fs = (float)S8 / 255.f;
  const float fv = (float)V;
  const int p = pm_aug_clip8((int)roundf(fv * (1.f - fs)));
  const int q = pm_aug_clip8((int)roundf(fv * (1.f - fs * f)));
  const int t = pm_aug_clip8((int)roundf(fv * (1.f - fs * (1.f - f))));
  switch (i % 6) {
    case 0: *r = V, *g = t, *b = p; break;
    case 1: *r = q, *g = V, *b = p; break;
    case 2: *r = p, *g = V, *b = t; break;
    case 3: *r = p, *g = q, *b = V; break;
    case 4: *r = t, *g = p, *b = V; break;
    default: *r = V, *g = p, *b = q; break;
  }
}

// The colour ops of one image in its own order, stopping in front of op `stop` (PM_AUG_CONTRAST: the state the grey sum is taken in; 4: all of them).
// `mean`: the rounded grey mean of that state over the whole image.
PM_AUG_HD void pm_aug_colour(int* r, int* g, int* b, const pm_aug_image& P, int mean, int stop) {
  for (int k = 0; k < 4; ++k) {
    const int op = P.order[k];
    if (op == stop) return;
    if (!((P.enabled >> op) & 1)) continue;
    if (op == PM_AUG_BRIGHTNESS) {
      *r = pm_aug_blend(0, *r, P.brightness), *g = pm_aug_blend(0, *g, P.brightness), *b = pm_aug_blend(0, *b, P.brightness);
    } else if (op == PM_AUG_CONTRAST) {
      *r = pm_aug_blend(mean, *r, P.contrast), *g = pm_aug_blend(mean, *g, P.contrast), *b = pm_aug_blend(mean, *b, P.contrast);
    } else if (op == PM_AUG_SATURATION) {
      const int l = pm_aug_grey(*r, *g, *b);
      *r = pm_aug_blend(l, *r, P.saturation), *g = pm_aug_blend(l, *g, P.saturation), *b = pm_aug_blend(l, *b, P.saturation);
    } else if (op == PM_AUG_HUE) {
      int h8, s8;
      const int v = *r > *g ? (*r > *b ? *r : *b) : (*g > *b ? *g : *b);
      pm_aug_rgb2hsv(*r, *g, *b, &h8, &s8);
      pm_aug_hsv2rgb((h8 + P.hue_shift) & 255, s8, v, r, g, b);
    }
  }
}
// (int)(sum / count + 0.5) in double: ImageEnhance.Contrast's int(ImageStat.Stat(image.convert("L")).mean[0] + 0.5)
PM_AUG_HD int pm_aug_mean(unsigned long long sum, long count) { return (int)((double)sum / (double)count + 0.5); }
