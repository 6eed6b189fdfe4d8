/* lh2_filter.h - the SVGF denoise chain of the render core (setting "filter"): parameter blocks, launchers and the
   packed formats shared by the capture in shade_path (lh2_kernels.hip) and the filter kernels (lh2_filter.hip).

   The algorithm is Lighthouse 2's filtering core (finalize_shared.h prepareFilterKernel / applyFilterKernel, the capture
   of RenderCore_Optix7Filter's shade kernel), restated for this core.  Per frame:
     shade (capture)    features, worldPos, deltaDepth of each pixel's first non-specular vertex; direct and indirect
                        light in two accumulator planes
     k_filter_prepare   demodulate by albedo, clamp, pack direct + indirect into one float4; reproject; luminance moments
                        (a diffuse pixel moves by the difference of its vertex's screen positions in the previous and the
                        current view, so the sample's sub-pixel offset drops out: a still camera gives pixel + 0.5 exactly,
                        where the reference's vector carries the offset)
     k_filter_atrous    three edge-stopping a-trous passes (steps 1, 2, 4); the first also blends with the previous frame's
                        first-pass output, the last remodulates by albedo and writes the frame
   and, with the setting "TAA" on as well (TAApassKernel / unsharpenTAAKernel; the last pass then writes `linear`):
     k_filter_taa       temporal antialiasing in gamma space: the previous frame's TAA pixels at the motion vector
                        (Mitchell-Netravali), clamped in YCoCg to this frame's 3 x 3 neighbourhood, blended 0.9 : 0.1
     k_filter_unsharpen sharpens what TAA blurred, squares the gamma away and writes the frame
   Buffers (w x h records each):
     features  uint4   x: albedo 10:11:11; y: packed normal (PackNormal2) + specular bit; z: hit distance (float bits);
                       w: history count (bits 0-3), specular flag (bits 4-5), material id (from bit 6)
     worldPos  float4  xyz: position of that vertex; w: the packed normal again (bits)
     deltaDepth float4 zw: depth change towards pixel (x + 1, y) and (x, y + 1) along the hit triangle's plane
     motion    float2  the pixel's position in the previous frame (+ 0.5)
     moments   float4  luminance and squared luminance of direct and indirect light, blended over time
     shading and the pass outputs: float4 holding two rgb triples as 5:11 fixed point (filter_combine)
     linear    float4  TAA only: the last pass's output (linear radiance, w = 1)
     taa       float4  TAA only, a pair like the history pairs: sqrt of the antialiased radiance, at most 10, w = 0 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lh2_kernels.h"

#define LH2_FILTER_CLAMP_DIRECT 2.5f     /* the reference's defaults (rendercore.h DeviceVars) */
#define LH2_FILTER_CLAMP_INDIRECT 15.0f
#define LH2_FILTER_MISS_T 1e34f          /* features.z of a pixel whose path left the scene */

struct FilterPrepareArgs
{
	const float4* acc;               /* two planes of w x h: direct, indirect */
	uint4* features;                 /* w: the history count is bumped or reset */
	const float4* worldPos; const float4* prevWorldPos; const float4* deltaDepth;
	const float4* prevMoments;
	float4* shading; float2* motion; float4* moments;
	/* the previous and the current view (lh2_filter_view): position + plane term, view direction, pixel-scaled right and up */
	float4 prevView[4], curView[4];
	int w, h;
	float scale;                     /* 1 / samples per pixel in the accumulator */
	float clampDirect, clampIndirect;
	int camStationary;               /* specular pixels keep their position (no search) */
	int historyValid;                /* 0: the first frame after a reset (no previous buffers) */
};

struct FilterAtrousArgs
{
	const uint4* features; const float4* worldPos; const float4* prevWorldPos; const float4* deltaDepth;
	const float2* motion; const float4* moments;
	const float4* A;                 /* input (shading, or the previous pass) */
	const float4* B;                 /* phase 1: the previous frame's phase-1 output */
	float4* C;                       /* output; phase 3: the frame (linear radiance) */
	int w, h, phase;                 /* phase 1 .. 3: step 1, 2, 4; 3 is the last pass */
	int historyValid;
	int lds;                         /* taps from an LDS tile (1) or straight from memory through L1 / L2 (0) */
};

struct FilterTaaArgs   /* k_filter_taa and k_filter_unsharpen */
{
	const float4* in;                /* taa: the last pass's linear output; unsharpen: the taa pass's output */
	const float4* prev;              /* taa: the previous frame's taa output */
	const float2* motion;            /* taa */
	float4* out;                     /* never `in` or `prev`: both kernels read their neighbours */
	int w, h;
	int historyValid;                /* taa; 0: the pixel passes through */
	int lds;                         /* taa: the 3 x 3 neighbourhood from an LDS tile (1) or through L1 / L2 (0) */
};

extern "C" {
/* the reprojection constants of a view (prepareFilter's host part) */
void lh2_filter_view( const lh2_ViewPyramid* view, int h, float4 out[4] );
void lh2_launch_filter_prepare( const FilterPrepareArgs* a, LaunchEvents ev, hipStream_t st );
void lh2_launch_filter_atrous( const FilterAtrousArgs* a, LaunchEvents ev, hipStream_t st );
void lh2_launch_filter_taa( const FilterTaaArgs* a, LaunchEvents ev, hipStream_t st );
void lh2_launch_filter_unsharpen( const FilterTaaArgs* a, LaunchEvents ev, hipStream_t st );
}

/* ---- packed formats (tools_shared.h PackNormal2 / HDRtoRGB32 / CombineToFloat4 and their inverses) ---- */
#define LH2_FDEV static __device__ __forceinline__
LH2_FDEV uint32_t filter_f2u( const float f ) { return (uint32_t)fminf( fmaxf( f, 0.0f ), 4294967040.0f ); }   /* NaN and negatives: 0 */
LH2_FDEV uint32_t filter_pack_normal( const float x, const float y, const float z )
{
	const uint32_t ux = min( filter_f2u( (x + 1) * 511 ), 1023u ), uy = min( filter_f2u( (y + 1) * 511 ), 1023u ), uz = min( filter_f2u( (z + 1) * 511 ), 1023u );
	return (ux << 2) + (uy << 12) + (uz << 22);
}
LH2_FDEV void filter_unpack_normal( const uint32_t p, float& x, float& y, float& z )
{
	x = (float)((p >> 2) & 1023u) * (1.0f / 511.0f) - 1, y = (float)((p >> 12) & 1023u) * (1.0f / 511.0f) - 1, z = (float)(p >> 22) * (1.0f / 511.0f) - 1;
}
LH2_FDEV uint32_t filter_pack_rgb( const float r, const float g, const float b )
{
	return (filter_f2u( 1023.0f * fminf( 1.0f, r ) ) << 22) + (filter_f2u( 2047.0f * fminf( 1.0f, g ) ) << 11) + filter_f2u( 2047.0f * fminf( 1.0f, b ) );
}
LH2_FDEV void filter_unpack_rgb( const uint32_t c, float& r, float& g, float& b )
{
	r = (float)(c >> 22) * (1.0f / 1023.0f), g = (float)((c >> 11) & 2047u) * (1.0f / 2047.0f), b = (float)(c & 2047u) * (1.0f / 2047.0f);
}
LH2_FDEV uint32_t filter_features_w( const uint32_t old, const uint32_t isSpecular, const uint32_t matid )
{
	return (isSpecular << 4) + (matid << 6) + (old & 15u);   /* the history count stays */
}
