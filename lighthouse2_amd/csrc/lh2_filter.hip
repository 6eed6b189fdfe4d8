/* lh2_filter.hip - the SVGF filter kernels (lh2_filter.h): k_filter_prepare, k_filter_atrous<PHASE, LDS>, and the
   TAA stage k_filter_taa<LDS> / k_filter_unsharpen.

   The arithmetic restates Lighthouse 2's prepareFilterKernel / applyFilterKernel / TAApassKernel / unsharpenTAAKernel
   (finalize_shared.h) with their helpers (sampling_shared.h ReadTexelConsistent / ReadTexelConsistent2 /
   ReadTexelBmitchellNetravali, tools_shared.h); the file is compiled like the rest of the core (no FMA contraction),
   so tests/filter_ref.py and tests/taa_ref.py restate it operation by operation.  Left out: the TAA jitter
   (j0 = j1 = 0: DESIGN.md section 9).  The last pass writes linear radiance; the sqrt the reference's last pass takes
   for TAA is taken by k_filter_taa on load.  Where the TAA stage departs from the reference's text (an output buffer of
   its own, the bicubic footprint, the first frame, the frame's border): DESIGN.md section 9.

   The a-trous pass reads 21 taps of A and features (32 B each) per pixel; its unique traffic is 80 B per pixel.  A
   block filters a 32 x 8 tile; the LDS variant stages the tile with a halo of 2 x step pixels (36 x 12, 40 x 16,
   48 x 24 records of 32 B: 13.5, 20, 36 KiB), the other reads the taps through L1 / L2 (profiles/ *_ab_filter_lds.txt). */
#include <hip/hip_ext.h>
#include "lh2_filter.h"
#include "lh2_device.h"

#include <algorithm>
#include <cmath>

#define FILTER_TX 32
#define FILTER_TY 8

/* ---- helpers ---------------------------------------------------------------------------- */
LH2_DEV v3 unpack_n( const uint32_t p ) { v3 n; filter_unpack_normal( p, n.x, n.y, n.z ); return n; }
LH2_DEV v3 unpack_rgb( const uint32_t c ) { v3 r; filter_unpack_rgb( c, r.x, r.y, r.z ); return r; }
LH2_DEV v3 unpack_rgb_min1( const uint32_t c )   /* RGB32toHDRmin1: no zero channel (the albedo divides) */
{
	return mk3( (float)max( 1u, c >> 22 ) * (1.0f / 1023.0f), (float)max( 1u, (c >> 11) & 2047u ) * (1.0f / 2047.0f), (float)max( 1u, c & 2047u ) * (1.0f / 2047.0f) );
}
LH2_DEV float filter_lum( const v3 c ) { return 0.299f * fminf( c.x, 10.0f ) + 0.587f * fminf( c.y, 10.0f ) + 0.114f * fminf( c.z, 10.0f ); }
/* two rgb triples in one float4 as 5:11 unsigned fixed point (CombineToFloat4) */
LH2_DEV float4 filter_combine( const v3 a, const v3 b )
{
	const uint32_t ar = filter_f2u( fminf( a.x, 31.999f ) * 2048.0f ), ag = filter_f2u( fminf( a.y, 31.999f ) * 2048.0f ), ab = filter_f2u( fminf( a.z, 31.999f ) * 2048.0f );
	const uint32_t br = filter_f2u( fminf( b.x, 31.999f ) * 2048.0f ), bg = filter_f2u( fminf( b.y, 31.999f ) * 2048.0f ), bb = filter_f2u( fminf( b.z, 31.999f ) * 2048.0f );
	return make_float4( bitsf( (ar << 16) + ag ), bitsf( ab ), bitsf( (br << 16) + bg ), bitsf( bb ) );
}
LH2_DEV v3 filter_direct( const float4 c )
{
	const uint32_t v0 = fbits( c.x ), v1 = fbits( c.y );
	return mk3( (float)(v0 >> 16) * (1.0f / 2048.0f), (float)(v0 & 65535u) * (1.0f / 2048.0f), (float)v1 * (1.0f / 2048.0f) );
}
LH2_DEV v3 filter_indirect( const float4 c )
{
	const uint32_t v2 = fbits( c.z ), v3_ = fbits( c.w );
	return mk3( (float)(v2 >> 16) * (1.0f / 2048.0f), (float)(v2 & 65535u) * (1.0f / 2048.0f), (float)v3_ * (1.0f / 2048.0f) );
}
LH2_DEV v3 rgb_to_ycocg( const v3 c )
{
	const v3 r = mk3( fminf( 4.0f, c.x ), fminf( 4.0f, c.y ), fminf( 4.0f, c.z ) );
	const float k = 0.5f * 256.0f / 255.0f;
	return mk3( (r.x * 1 + r.y * 2 + r.z * 1) * 0.25f, (r.x * 2 + r.y * 0 + r.z * -2) * 0.25f + k, (r.x * -1 + r.y * 2 + r.z * -1) * 0.25f + k );
}
LH2_DEV v3 ycocg_to_rgb( const v3 c )
{
	const float k = 0.5f * 256.0f / 255.0f;
	const float Y = c.x, Co = c.y - k, Cg = c.z - k;
	return mk3( Y + Co - Cg, Y + Cg, Y - Co - Cg );
}
LH2_DEV float pow128( float x ) { x *= x, x *= x, x *= x, x *= x, x *= x, x *= x, x *= x; return x; }   /* x^128: seven squarings */
LH2_DEV v3 clamp3( const v3 v, const v3 lo, const v3 hi )
{
	return mk3( fminf( fmaxf( v.x, lo.x ), hi.x ), fminf( fmaxf( v.y, lo.y ), hi.y ), fminf( fmaxf( v.z, lo.z ), hi.z ) );
}

/* the four texels around (u, v) of the previous frame with their bilinear weights; a tap whose normal or specular
   bit differs from the pixel's gets weight 0 (ReadTexelConsistent*, the reference's 'relax' branch: the world
   distance is left to the neighbourhood clamp).  False: outside the frame */
struct HistoryTaps { int i0, i1, i2, i3; float w0, w1, w2, w3; };
LH2_DEV bool history_taps( const float4* __restrict__ prevWorldPos, const uint32_t localBits, const v3 localNormal, const float minDot,
	const float u, const float v, const int w, const int h, HistoryTaps& t )
{
	const float fu = floorf( u ), fv = floorf( v );
	const int iu1 = (int)fu, iv1 = (int)fv, iu0 = max( 0, iu1 - 1 ), iv0 = max( 0, iv1 - 1 );
	if (iu1 >= w || iv1 >= h || iu1 < 0 || iv1 < 0) return false;
	const float fx = u - fu, fy = v - fv;
	t.i0 = iu0 + iv0 * w, t.i1 = iu1 + iv0 * w, t.i2 = iu0 + iv1 * w, t.i3 = iu1 + iv1 * w;
	t.w0 = (1 - fx) * (1 - fy), t.w1 = fx * (1 - fy), t.w2 = (1 - fx) * fy, t.w3 = 1 - (t.w0 + t.w1 + t.w2);
	const uint32_t n0 = fbits( prevWorldPos[t.i0].w ), n1 = fbits( prevWorldPos[t.i1].w ), n2 = fbits( prevWorldPos[t.i2].w ), n3 = fbits( prevWorldPos[t.i3].w );
	const uint32_t spec = localBits & 3u;
	if (dot3( unpack_n( n0 ), localNormal ) < minDot || (n0 & 3u) != spec) t.w0 = 0;
	if (dot3( unpack_n( n1 ), localNormal ) < minDot || (n1 & 3u) != spec) t.w1 = 0;
	if (dot3( unpack_n( n2 ), localNormal ) < minDot || (n2 & 3u) != spec) t.w2 = 0;
	if (dot3( unpack_n( n3 ), localNormal ) < minDot || (n3 & 3u) != spec) t.w3 = 0;
	return true;
}

/* ---- the specular pixels' search for their previous position (RefineHistoryPos) ----------- */
LH2_DEV float world_distance( const int px, const int py, const float4 cur, const float4* __restrict__ prevWorldPos, const int w, const int h )
{
	float4 p = make_float4( 1e20f, 1e20f, 1e20f, 0.0f );
	if (px >= 0 && py >= 0 && px < w && py < h) p = prevWorldPos[px + py * w];
	if ((fbits( p.w ) & 3u) != 1u) return 1e21f;   /* specular pixels only */
	if (dot3( unpack_n( fbits( cur.w ) ), unpack_n( fbits( p.w ) ) ) < 0.85f) return 1e21f;
	return length3( mk3( cur.x - p.x, cur.y - p.y, cur.z - p.z ) );
}
LH2_DEV float fine_world_distance( const float px, const float py, const float4 cur, const float4* __restrict__ prevWorldPos, const int w, const int h )
{
	const int x0 = (int)px, y0 = (int)py;
	const float fx = px - floorf( px ), fy = py - floorf( py );
	const float w0 = (1 - fx) * (1 - fy), w1 = fx * (1 - fy), w2 = (1 - fx) * fy, w3 = fx * fy;
	const float d0 = world_distance( x0, y0, cur, prevWorldPos, w, h ), d1 = world_distance( x0 + 1, y0, cur, prevWorldPos, w, h );
	const float d2 = world_distance( x0, y0 + 1, cur, prevWorldPos, w, h ), d3 = world_distance( x0 + 1, y0 + 1, cur, prevWorldPos, w, h );
	float totalWeight = 0, totalDist = 0;
	if (d0 < 1e20f) totalDist += d0 * w0, totalWeight += w0;
	if (d1 < 1e20f) totalDist += d1 * w1, totalWeight += w1;
	if (d2 < 1e20f) totalDist += d2 * w2, totalWeight += w2;
	if (d3 < 1e20f) totalDist += d3 * w3, totalWeight += w3;
	return totalWeight == 0 ? 1e20f : totalDist / totalWeight;
}

/* a world position on the screen of a view (lh2_filter_view), in pixels from its top-left corner */
LH2_DEV void view_project( const float4* __restrict__ v, const float4 wp, float& px, float& py )
{
	const float4 pos = v[0], E = v[1], R = v[2], U = v[3];
	const v3 D = normalize3( mk3( wp.x - pos.x, wp.y - pos.y, wp.z - pos.z ) );
	const float t = pos.w / dot3( xyz( E ), D );
	const v3 S = add3( xyz( pos ), muls( D, t ) );
	px = dot3( S, xyz( R ) ) - R.w, py = dot3( S, xyz( U ) ) - U.w;
}

/* ---- k_filter_prepare ---------------------------------------------------------------------- */
__global__ __launch_bounds__( 256 ) void k_filter_prepare( const FilterPrepareArgs a )
{
	const int x = (int)(threadIdx.x + blockIdx.x * FILTER_TX), y = (int)(threadIdx.y + blockIdx.y * FILTER_TY);
	const int w = a.w, h = a.h;
	if (x >= w || y >= h) return;
	const int pixelIdx = x + y * w;
	/* albedo out of the light, clamped */
	const float4 acc0 = a.acc[pixelIdx], acc1 = a.acc[pixelIdx + w * h];
	const uint4 localFeature = a.features[pixelIdx];
	const float4 localWorldPos = a.worldPos[pixelIdx];
	const v3 albedo = unpack_rgb_min1( localFeature.x );
	const v3 direct = muls( xyz( acc0 ), a.scale ), indirect = muls( xyz( acc1 ), a.scale );
	const v3 reciAlbedo = mk3( 1.0f / albedo.x, 1.0f / albedo.y, 1.0f / albedo.z );
	const v3 dl = mul3( direct, reciAlbedo ), il = mul3( indirect, reciAlbedo );
	const v3 directLight = mk3( fminf( dl.x, a.clampDirect ), fminf( dl.y, a.clampDirect ), fminf( dl.z, a.clampDirect ) );
	const v3 indirectLight = mk3( fminf( il.x, a.clampIndirect ), fminf( il.y, a.clampIndirect ), fminf( il.z, a.clampIndirect ) );
	a.shading[pixelIdx] = filter_combine( directLight, indirectLight );
	float lumDirect = filter_lum( directLight ), lumDirect2 = lumDirect * lumDirect;
	float lumIndirect = filter_lum( indirectLight ), lumIndirect2 = lumIndirect * lumIndirect;
	/* where this pixel was in the previous frame */
	float ppx, ppy;
	if (((localFeature.w >> 4) & 3u) == 0)
	{
		/* diffuse: its world position through the previous view, less where the current view has it (the sample's place in
		   the pixel: the difference is the pixel's motion, exactly zero for equal views) */
		float px0, py0, px1, py1;
		view_project( a.prevView, localWorldPos, px0, py0 );
		view_project( a.curView, localWorldPos, px1, py1 );
		ppx = (float)x + (px0 - px1), ppy = (float)y + (py0 - py1);
	}
	else
	{
		ppx = (float)x, ppy = (float)y;
		if (!a.camStationary && a.historyValid)
		{
			/* specular: a diamond search over the previous frame's world positions */
			const float4 pw = a.prevWorldPos[pixelIdx];
			float bestDist = length3( mk3( localWorldPos.x - pw.x, localWorldPos.y - pw.y, localWorldPos.z - pw.z ) ), stepSize = 5.0f;
			for (int iter = 0; iter < 25; iter++)
			{
				const float cx = ppx, cy = ppy;
				int tap = 0;
				float d;
				d = fine_world_distance( cx - stepSize, cy, localWorldPos, a.prevWorldPos, w, h );
				if (d < bestDist) bestDist = d, ppx = cx - stepSize, ppy = cy, tap = 1;
				d = fine_world_distance( cx + stepSize, cy, localWorldPos, a.prevWorldPos, w, h );
				if (d < bestDist) bestDist = d, ppx = cx + stepSize, ppy = cy, tap = 2;
				d = fine_world_distance( cx, cy - stepSize, localWorldPos, a.prevWorldPos, w, h );
				if (d < bestDist) bestDist = d, ppx = cx, ppy = cy - stepSize, tap = 3;
				d = fine_world_distance( cx, cy + stepSize, localWorldPos, a.prevWorldPos, w, h );
				if (d < bestDist) bestDist = d, ppx = cx, ppy = cy + stepSize, tap = 4;
				if (tap == 0) { stepSize *= 0.45f; if (stepSize < 0.05f) break; }
			}
		}
	}
	ppx += 0.5f, ppy += 0.5f;
	/* the history's luminance moments, if the pixel was there */
	bool found = false;
	if (a.historyValid && ppx >= 0 && ppx < (float)w && ppy >= 0 && ppy < (float)h)
	{
		HistoryTaps t;
		if (history_taps( a.prevWorldPos, fbits( localWorldPos.w ), unpack_n( localFeature.y ), 0.95f, ppx, ppy, w, h, t ))
		{
			const float sum = t.w0 + t.w1 + t.w2 + t.w3;
			if (sum != 0)
			{
				const float4 p0 = a.prevMoments[t.i0], p1 = a.prevMoments[t.i1], p2 = a.prevMoments[t.i2], p3 = a.prevMoments[t.i3];
				const float rs = 1.0f / sum;
				const float hx = (t.w0 * p0.x + t.w1 * p1.x + t.w2 * p2.x + t.w3 * p3.x) * rs, hy = (t.w0 * p0.y + t.w1 * p1.y + t.w2 * p2.y + t.w3 * p3.y) * rs;
				const float hz = (t.w0 * p0.z + t.w1 * p1.z + t.w2 * p2.z + t.w3 * p3.z) * rs, hw = (t.w0 * p0.w + t.w1 * p1.w + t.w2 * p2.w + t.w3 * p3.w) * rs;
				if (hx > -1)
				{
					lumDirect = 0.2f * lumDirect + 0.8f * hx, lumDirect2 = 0.2f * lumDirect2 + 0.8f * hy;
					lumIndirect = 0.2f * lumIndirect + 0.8f * hz, lumIndirect2 = 0.2f * lumIndirect2 + 0.8f * hw;
					found = true;
				}
			}
		}
	}
	uint32_t fw = localFeature.w;
	if (found) { if ((fw & 15u) < 15u) fw++; } else fw &= 0xfffffff0u;
	a.features[pixelIdx].w = fw;
	a.motion[pixelIdx] = make_float2( ppx, ppy );
	a.moments[pixelIdx] = make_float4( lumDirect, lumDirect2, lumIndirect, lumIndirect2 );
}

/* ---- k_filter_atrous ------------------------------------------------------------------------ */
template <int PHASE> struct AtrousTile
{
	static constexpr int STEP = 1 << (PHASE - 1), HALO = 2 * STEP;
	static constexpr int W = FILTER_TX + 2 * HALO, H = FILTER_TY + 2 * HALO;
};

template <int PHASE, bool LDS>
__global__ __launch_bounds__( 256 ) void k_filter_atrous( const FilterAtrousArgs a )
{
	using Tile = AtrousTile<PHASE>;
	constexpr int STEP = Tile::STEP, HALO = Tile::HALO;
	constexpr bool LAST = PHASE == 3;
	const int w = a.w, h = a.h;
	const int bx0 = (int)blockIdx.x * FILTER_TX, by0 = (int)blockIdx.y * FILTER_TY;
	const int x = bx0 + (int)threadIdx.x, y = by0 + (int)threadIdx.y;
	__shared__ float4 sA[LDS ? Tile::W * Tile::H : 1];
	__shared__ uint4 sF[LDS ? Tile::W * Tile::H : 1];
	if (LDS)
	{
		/* the tile with its halo: columns clamped to the frame (the taps' own clamp), rows outside it left out (never read) */
		for (int i = (int)(threadIdx.y * FILTER_TX + threadIdx.x); i < Tile::W * Tile::H; i += FILTER_TX * FILTER_TY)
		{
			const int ty = i / Tile::W, tx = i - ty * Tile::W;
			const int gx = min( max( bx0 - HALO + tx, 0 ), w - 1 ), gy = by0 - HALO + ty;
			if (gy >= 0 && gy < h) sA[i] = a.A[gx + gy * w], sF[i] = a.features[gx + gy * w];
		}
		__syncthreads();
	}
	if (x >= w || y >= h) return;
	const int pixelIdx = x + y * w;
	const int lc = ((int)threadIdx.y + HALO) * Tile::W + (int)threadIdx.x + HALO;   /* the pixel's tile cell */
	/* the pixel */
	const uint4 localFeature = LDS ? sF[lc] : a.features[pixelIdx];
	const float4 combined = LDS ? sA[lc] : a.A[pixelIdx];
	const float4 dd = a.deltaDepth[pixelIdx];
	const float4 m = a.moments[pixelIdx];
	const v3 localNormal = unpack_n( localFeature.y );
	const v3 localColor = unpack_rgb( localFeature.x );
	const uint32_t localMatID = localFeature.w >> 4;
	float directWeightSum = 1, indirectWeightSum = 1;
	v3 directSum = filter_direct( combined ), indirectSum = filter_indirect( combined );
	const float localDirect = filter_lum( directSum ), localIndirect = filter_lum( indirectSum );
	const float localDepth = bitsf( localFeature.z );
	const float localDdx = dd.z, localDdy = dd.w;
	/* luminance weights scaled by the moments' variance; without history they barely count (x 400) */
	const float sigma = 10.0f * bitsf( (uint32_t)(127 - (PHASE - 1)) << 23 );
	const float factor = (localFeature.w & 15u) == 0 ? 400.0f : 1.0f;
	const float varDir = m.y - m.x * m.x, varInd = m.w - m.z * m.z;
	const float reciDir = -1.0f / (sigma * factor * sqrtf( varDir + 0.00001f ) + 0.00001f);
	const float reciInd = -1.0f / (sigma * factor * sqrtf( varInd + 0.00001f ) + 0.00001f);
	const float depthScale = 0.5f + (float)PHASE * 0.5f;
	/* the 5 x 5 footprint without its corners */
#pragma unroll
	for (int vv = -2; vv <= 2; vv++)
	{
		const int v = vv * STEP + y;
		const int r = (vv == 2 || vv == -2) ? 1 : 2;
		if (v >= 0 && v < h)
		{
#pragma unroll
			for (int uu = -r; uu <= r; uu++) if (uu != 0 || vv != 0)
			{
				float4 nc; uint4 nf;
				if (LDS)
				{
					const int c = lc + vv * STEP * Tile::W + uu * STEP;
					nc = sA[c], nf = sF[c];
				}
				else
				{
					const int u = min( max( uu * STEP + x, 0 ), w - 1 );
					nc = a.A[u + v * w], nf = a.features[u + v * w];
				}
				const float wDist = (float)(uu * uu + vv * vv) * (-1.0f / 7.5f);
				const v3 nDirect = filter_direct( nc ), nIndirect = filter_indirect( nc );
				float wNormal = pow128( fmaxf( 0.0f, dot3( unpack_n( nf.y ), localNormal ) ) );
				/* depth along the pixel's plane; not too strict, curved surfaces */
				const float expected = localDepth + localDdx * (float)(uu * STEP) + localDdy * (float)(vv * STEP);
				const float depthError = fabsf( expected - bitsf( nf.z ) );
				const float expectedDiff = fabsf( expected - localDepth );
				const float wDepth = depthError / fmaxf( 0.00001f, depthScale * expectedDiff );
				/* other materials hardly count; the same one by its albedo */
				wNormal *= (nf.w >> 4) != localMatID ? 0.0001f : dot3( localColor, unpack_rgb( nf.x ) );
				float wDir = wNormal * __expf( fabsf( localDirect - filter_lum( nDirect ) ) * reciDir + wDist - wDepth );
				float wInd = wNormal * __expf( fabsf( localIndirect - filter_lum( nIndirect ) ) * reciInd + wDist - wDepth );
				if (!isfinite_( wDir )) wDir = 0;
				if (!isfinite_( wInd )) wInd = 0;
				directSum = add3( directSum, muls( nDirect, wDir ) ), directWeightSum += wDir;
				indirectSum = add3( indirectSum, muls( nIndirect, wInd ) ), indirectWeightSum += wInd;
			}
		}
	}
	v3 directFiltered = muls( directSum, 1.0f / fmaxf( 0.0001f, directWeightSum ) );
	v3 indirectFiltered = muls( indirectSum, 1.0f / fmaxf( 0.0001f, indirectWeightSum ) );
	if (PHASE == 1 && a.historyValid)
	{
		/* blend with the previous frame's first pass at the motion vector, clamped to this frame's 3 x 3 neighbourhood */
		const float2 prevPixelPos = a.motion[pixelIdx];
		const int px = (int)prevPixelPos.x, py = (int)prevPixelPos.y;
		HistoryTaps t;
		if (px >= 0 && px < w && py >= 0 && py < h &&
			history_taps( a.prevWorldPos, fbits( a.worldPos[pixelIdx].w ), localNormal, 0.975f, prevPixelPos.x, prevPixelPos.y, w, h, t ))
		{
			const float sum = t.w0 + t.w1 + t.w2 + t.w3;
			if (sum != 0)
			{
				const float4 b0 = a.B[t.i0], b1 = a.B[t.i1], b2 = a.B[t.i2], b3 = a.B[t.i3];
				const float rs = 1.0f / sum;
				v3 prevDirect = muls( add3( add3( add3( smul( t.w0, filter_direct( b0 ) ), smul( t.w1, filter_direct( b1 ) ) ), smul( t.w2, filter_direct( b2 ) ) ), smul( t.w3, filter_direct( b3 ) ) ), rs );
				v3 prevIndirect = muls( add3( add3( add3( smul( t.w0, filter_indirect( b0 ) ), smul( t.w1, filter_indirect( b1 ) ) ), smul( t.w2, filter_indirect( b2 ) ) ), smul( t.w3, filter_indirect( b3 ) ) ), rs );
				if (prevDirect.x != -1)
				{
					prevDirect = rgb_to_ycocg( prevDirect ), prevIndirect = rgb_to_ycocg( prevIndirect );
					v3 dirAvg = rgb_to_ycocg( directFiltered ), dirVar = mul3( dirAvg, dirAvg );
					v3 indAvg = rgb_to_ycocg( indirectFiltered ), indVar = mul3( indAvg, indAvg );
					/* the neighbours that take part (the reference's bounds: x > 1, y > 1 on the low side) */
					auto tap = [&]( const int dx, const int dy ) {
						const float4 c4 = LDS ? sA[lc + dy * Tile::W + dx] : a.A[pixelIdx + dy * w + dx];
						const v3 f = rgb_to_ycocg( filter_direct( c4 ) ), g = rgb_to_ycocg( filter_indirect( c4 ) );
						dirAvg = add3( dirAvg, f ), dirVar = add3( dirVar, mul3( f, f ) ), indAvg = add3( indAvg, g ), indVar = add3( indVar, mul3( g, g ) );
					};
					if (x > 1)
					{
						if (y > 1) tap( -1, -1 );
						tap( -1, 0 );
						if (y < h - 1) tap( -1, 1 );
					}
					if (y > 1) tap( 0, -1 );
					if (y < h - 1) tap( 0, 1 );
					if (x < w - 1)
					{
						if (y > 1) tap( 1, -1 );
						tap( 1, 0 );
						if (y < h - 1) tap( 1, 1 );
					}
					const float k9 = 1.0f / 9.0f;
					dirAvg = muls( dirAvg, k9 ), dirVar = muls( dirVar, k9 ), indAvg = muls( indAvg, k9 ), indVar = muls( indVar, k9 );
					const v3 vd = sub3( dirVar, mul3( dirAvg, dirAvg ) ), vi = sub3( indVar, mul3( indAvg, indAvg ) );
					const v3 sigmaDir = mk3( sqrtf( fmaxf( 0.0f, vd.x ) ), sqrtf( fmaxf( 0.0f, vd.y ) ), sqrtf( fmaxf( 0.0f, vd.z ) ) );
					const v3 sigmaInd = mk3( sqrtf( fmaxf( 0.0f, vi.x ) ), sqrtf( fmaxf( 0.0f, vi.y ) ), sqrtf( fmaxf( 0.0f, vi.z ) ) );
					prevDirect = clamp3( prevDirect, sub3( dirAvg, smul( 0.75f, sigmaDir ) ), add3( dirAvg, smul( 0.75f, sigmaDir ) ) );
					prevIndirect = clamp3( prevIndirect, sub3( indAvg, smul( 0.75f, sigmaInd ) ), add3( indAvg, smul( 0.75f, sigmaInd ) ) );
					directFiltered = add3( muls( directFiltered, 0.1f ), muls( ycocg_to_rgb( prevDirect ), 0.9f ) );
					indirectFiltered = add3( muls( indirectFiltered, 0.1f ), muls( ycocg_to_rgb( prevIndirect ), 0.9f ) );
				}
			}
		}
	}
	if (LAST)
	{
		/* albedo back in; linear radiance, as k_finalize writes it */
		const v3 c = mul3( add3( directFiltered, indirectFiltered ), localColor );
		a.C[pixelIdx] = make_float4( c.x, c.y, c.z, 1.0f );
	}
	else a.C[pixelIdx] = filter_combine( directFiltered, indirectFiltered );
}

/* ---- k_filter_taa / k_filter_unsharpen (setting "TAA") --------------------------------------- */
/* both read a pixel's 3 x 3 neighbourhood.  The TAA pass converts each neighbour (sqrt, YCoCg): its LDS variant stages the
   block's 32 x 8 tile with a halo of one pixel, converted once.  A thread stages its own pixel's cell, the block's first 84
   threads one halo cell each as well; cells outside the frame are left out (never read).  The unsharpen reads its
   neighbours as they are, through L1 / L2: a tile buys it nothing (profiles/ *_ab_taa_lds.txt) */
#define TAA_TW (FILTER_TX + 2)
#define TAA_TH (FILTER_TY + 2)
LH2_DEV bool taa_halo_cell( const int t, int& tx, int& ty )
{
	if (t < TAA_TW) tx = t, ty = 0;
	else if (t < 2 * TAA_TW) tx = t - TAA_TW, ty = TAA_TH - 1;
	else if (t < 2 * TAA_TW + FILTER_TY) tx = 0, ty = t - 2 * TAA_TW + 1;
	else if (t < 2 * TAA_TW + 2 * FILTER_TY) tx = TAA_TW - 1, ty = t - 2 * TAA_TW - FILTER_TY + 1;
	else return false;
	return true;
}
LH2_DEV float mitchell_netravali( const float v )   /* B = C = 1/3 */
{
	const float B = 1.0f / 3.0f, C = 1.0f / 3.0f, x = fabsf( v ), x2 = x * x, x3 = x2 * x;
	if (x < 1) return (1.0f / 6.0f) * ((12 - 9 * B - 6 * C) * x3 + (-18 + 12 * B + 6 * C) * x2 + (6 - 2 * B));
	if (x < 2) return (1.0f / 6.0f) * ((-B - 6 * C) * x3 + (6 * B + 30 * C) * x2 + (-12 * B - 48 * C) * x + (8 * B + 24 * C));
	return 0.0f;
}
LH2_DEV v3 gamma3( const float4 c ) { return mk3( sqrtf( c.x ), sqrtf( c.y ), sqrtf( c.z ) ); }
LH2_DEV float4 taa_cell( const float4 linear ) { const v3 c = rgb_to_ycocg( gamma3( linear ) ); return make_float4( c.x, c.y, c.z, 0.0f ); }

/* temporal antialiasing of the filtered frame (TAApassKernel): in gamma space, the previous frame's result at the motion
   vector (Mitchell-Netravali), clamped in YCoCg to this frame's 3 x 3 neighbourhood, 0.9 of it against 0.1 of the pixel.
   Reads the last pass's linear output, writes gamma pixels to a buffer of its own (the next frame's history) */
template <bool LDS>
__global__ __launch_bounds__( 256 ) void k_filter_taa( const FilterTaaArgs a )
{
	const int w = a.w, h = a.h;
	const int bx0 = (int)blockIdx.x * FILTER_TX, by0 = (int)blockIdx.y * FILTER_TY;
	const int x = bx0 + (int)threadIdx.x, y = by0 + (int)threadIdx.y;
	const bool inFrame = x < w && y < h;
	const int pixelIdx = x + y * w;
	const int lc = ((int)threadIdx.y + 1) * TAA_TW + (int)threadIdx.x + 1;   /* the pixel's tile cell */
	__shared__ float4 sY[LDS ? TAA_TW * TAA_TH : 1];   /* the neighbourhood in YCoCg */
	v3 g = s3( 0.0f ), newPixel = s3( 0.0f );
	if (inFrame) g = gamma3( a.in[pixelIdx] ), newPixel = rgb_to_ycocg( g );
	if (LDS)
	{
		if (inFrame) sY[lc] = make_float4( newPixel.x, newPixel.y, newPixel.z, 0.0f );
		int tx, ty;
		if (taa_halo_cell( (int)(threadIdx.y * FILTER_TX + threadIdx.x), tx, ty ))
		{
			const int gx = bx0 - 1 + tx, gy = by0 - 1 + ty;
			if (gx >= 0 && gx < w && gy >= 0 && gy < h) sY[ty * TAA_TW + tx] = taa_cell( a.in[gx + gy * w] );
		}
		__syncthreads();
	}
	if (!inFrame) return;
	v3 pixel = g;
	const float2 m = a.motion[pixelIdx];
	const float u = m.x - 0.5f, v = m.y - 0.5f;
	if (a.historyValid && u >= 0 && u < (float)w && v >= 0 && v < (float)h)
	{
		/* the history: the kernel's support, floor( u ) - 1 .. floor( u ) + 2 per axis; taps outside the frame are skipped
		   and the weights renormalised */
		const int x1 = (int)floorf( u ) - 1, y1 = (int)floorf( v ) - 1;
		float wx[4], wy[4];
#pragma unroll
		for (int i = 0; i < 4; i++) wx[i] = mitchell_netravali( (float)(x1 + i) - u ), wy[i] = mitchell_netravali( (float)(y1 + i) - v );
		float totalWeight = 0;
		v3 total = s3( 0.0f );
#pragma unroll
		for (int j = 0; j < 4; j++)
		{
			const int ty = y1 + j;
			if (ty >= 0 && ty < h)
			{
#pragma unroll
				for (int i = 0; i < 4; i++)
				{
					const int tx = x1 + i;
					if (tx >= 0 && tx < w)
					{
						const float weight = wx[i] * wy[j];
						total = add3( total, muls( xyz( a.prev[tx + ty * w] ), weight ) );
						totalWeight += weight;
					}
				}
			}
		}
		const v3 historyRgb = muls( total, 1.0f / totalWeight );
		v3 history = rgb_to_ycocg( historyRgb );
		/* the neighbours that take part (the reference's bounds: x > 1, y > 1 on the low side; / 9 whatever their number) */
		v3 colorAvg = newPixel, colorVar = mul3( newPixel, newPixel );
		auto tap = [&]( const int dx, const int dy ) {
			const v3 f = LDS ? xyz( sY[lc + dy * TAA_TW + dx] ) : xyz( taa_cell( a.in[pixelIdx + dy * w + dx] ) );
			colorAvg = add3( colorAvg, f ), colorVar = add3( colorVar, mul3( f, f ) );
		};
		if (x > 1)
		{
			if (y > 1) tap( -1, -1 );
			tap( -1, 0 );
			if (y < h - 1) tap( -1, 1 );
		}
		if (y > 1) tap( 0, -1 );
		if (y < h - 1) tap( 0, 1 );
		if (x < w - 1)
		{
			if (y > 1) tap( 1, -1 );
			tap( 1, 0 );
			if (y < h - 1) tap( 1, 1 );
		}
		const float k9 = 1.0f / 9.0f;
		colorAvg = muls( colorAvg, k9 ), colorVar = muls( colorVar, k9 );
		const v3 var = sub3( colorVar, mul3( colorAvg, colorAvg ) );
		const v3 sigma = mk3( sqrtf( fmaxf( 0.0f, var.x ) ), sqrtf( fmaxf( 0.0f, var.y ) ), sqrtf( fmaxf( 0.0f, var.z ) ) );
		history = clamp3( history, sub3( colorAvg, smul( 1.25f, sigma ) ), add3( colorAvg, smul( 1.25f, sigma ) ) );
		pixel = ycocg_to_rgb( add3( muls( newPixel, 0.1f ), muls( history, 0.9f ) ) );
		/* NaN: the pixel without its history.  The history's own sum is tested as well: rgb_to_ycocg's fminf( 4, . ) turns a NaN
		   history into 4 before the blend's sum (the reference's only test) could show it */
		const float s = pixel.x + pixel.y + pixel.z, hs = historyRgb.x + historyRgb.y + historyRgb.z;
		if (s != s || hs != hs) pixel = ycocg_to_rgb( newPixel );
	}
	a.out[pixelIdx] = make_float4( fminf( 10.0f, pixel.x ), fminf( 10.0f, pixel.y ), fminf( 10.0f, pixel.z ), 0.0f );
}

/* what TAA blurred, sharpened again (unsharpenTAAKernel), and the gamma taken back: reads the TAA pass's pixels, writes the
   frame (linear radiance, w = 1).  The frame's border pixels have no full neighbourhood: they are only squared */
__global__ __launch_bounds__( 256 ) void k_filter_unsharpen( const FilterTaaArgs a )
{
	const int w = a.w, h = a.h;
	const int x = (int)(threadIdx.x + blockIdx.x * FILTER_TX), y = (int)(threadIdx.y + blockIdx.y * FILTER_TY);
	if (x >= w || y >= h) return;
	const int pixelIdx = x + y * w;
	v3 pixel = xyz( a.in[pixelIdx] );
	if (x > 0 && y > 0 && x < w - 1 && y < h - 1)
	{
		auto tap = [&]( const int dx, const int dy ) { return xyz( a.in[pixelIdx + dy * w + dx] ); };
		const v3 p0 = tap( -1, -1 ), p1 = tap( 0, -1 ), p2 = tap( 1, -1 ), p3 = tap( 1, 0 ), p4 = tap( 1, 1 ), p5 = tap( 0, 1 ), p6 = tap( -1, 1 ), p7 = tap( -1, 0 );
		v3 sum = add3( smul( 0.35f, p0 ), smul( 0.5f, p1 ) );
		sum = add3( sum, smul( 0.35f, p2 ) ), sum = add3( sum, smul( 0.5f, p3 ) ), sum = add3( sum, smul( 0.35f, p4 ) );
		sum = add3( sum, smul( 0.5f, p5 ) ), sum = add3( sum, smul( 0.35f, p6 ) ), sum = add3( sum, smul( 0.5f, p7 ) );
		const v3 sharp = sub3( muls( pixel, 2.7f ), smul( 0.5f, sum ) );
		pixel = mk3( fmaxf( pixel.x, sharp.x ), fmaxf( pixel.y, sharp.y ), fmaxf( pixel.z, sharp.z ) );
	}
	a.out[pixelIdx] = make_float4( pixel.x * pixel.x, pixel.y * pixel.y, pixel.z * pixel.z, 1.0f );
}

/* ---- launchers -------------------------------------------------------------------------- */
#define LH2_FLAUNCH( kernel, grid, block, st, ev, ... ) \
	hipExtLaunchKernelGGL( kernel, grid, block, 0, st, (ev).start, (ev).stop, 0, __VA_ARGS__ )

extern "C" {
void lh2_filter_view( const lh2_ViewPyramid* view, int h, float4 out[4] )
{
	auto sub = []( lh2_float3 a, lh2_float3 b ) { return lh2_float3{ a.x - b.x, a.y - b.y, a.z - b.z }; };
	auto dot = []( lh2_float3 a, lh2_float3 b ) { return a.x * b.x + a.y * b.y + a.z * b.z; };
	auto norm = [&]( lh2_float3 a ) { const float r = 1.0f / sqrtf( dot( a, a ) ); return lh2_float3{ a.x * r, a.y * r, a.z * r }; };
	const lh2_ViewPyramid& v = *view;
	const lh2_float3 centre = { 0.5f * (v.p2.x + v.p3.x), 0.5f * (v.p2.y + v.p3.y), 0.5f * (v.p2.z + v.p3.z) };
	const lh2_float3 direction = norm( sub( centre, v.pos ) ), right = norm( sub( v.p2, v.p1 ) ), up = norm( sub( v.p3, v.p1 ) );
	const lh2_float3 d31 = sub( v.p3, v.p1 );
	const float lenReci = (float)h / sqrtf( dot( d31, d31 ) );
	out[0] = make_float4( v.pos.x, v.pos.y, v.pos.z, -(dot( v.pos, direction ) - dot( centre, direction )) );
	out[1] = make_float4( direction.x, direction.y, direction.z, 0 );
	out[2] = make_float4( right.x * lenReci, right.y * lenReci, right.z * lenReci, dot( v.p1, right ) * lenReci );
	out[3] = make_float4( up.x * lenReci, up.y * lenReci, up.z * lenReci, dot( v.p1, up ) * lenReci );
}
static dim3 filter_grid( int w, int h ) { return dim3( (unsigned)((w + FILTER_TX - 1) / FILTER_TX), (unsigned)((h + FILTER_TY - 1) / FILTER_TY) ); }
void lh2_launch_filter_prepare( const FilterPrepareArgs* a, LaunchEvents ev, hipStream_t st )
{
	LH2_FLAUNCH( k_filter_prepare, filter_grid( a->w, a->h ), dim3( FILTER_TX, FILTER_TY ), st, ev, *a );
}
void lh2_launch_filter_atrous( const FilterAtrousArgs* a, LaunchEvents ev, hipStream_t st )
{
	const dim3 g = filter_grid( a->w, a->h ), b( FILTER_TX, FILTER_TY );
	switch (a->phase * 2 + (a->lds ? 1 : 0))
	{
	case 2: LH2_FLAUNCH( (k_filter_atrous<1, false>), g, b, st, ev, *a ); break;
	case 3: LH2_FLAUNCH( (k_filter_atrous<1, true>), g, b, st, ev, *a ); break;
	case 4: LH2_FLAUNCH( (k_filter_atrous<2, false>), g, b, st, ev, *a ); break;
	case 5: LH2_FLAUNCH( (k_filter_atrous<2, true>), g, b, st, ev, *a ); break;
	case 6: LH2_FLAUNCH( (k_filter_atrous<3, false>), g, b, st, ev, *a ); break;
	case 7: LH2_FLAUNCH( (k_filter_atrous<3, true>), g, b, st, ev, *a ); break;
	default: break;   /* the host passes phases 1 .. 3 only */
	}
}
void lh2_launch_filter_taa( const FilterTaaArgs* a, LaunchEvents ev, hipStream_t st )
{
	const dim3 g = filter_grid( a->w, a->h ), b( FILTER_TX, FILTER_TY );
	if (a->lds) LH2_FLAUNCH( k_filter_taa<true>, g, b, st, ev, *a ); else LH2_FLAUNCH( k_filter_taa<false>, g, b, st, ev, *a );
}
void lh2_launch_filter_unsharpen( const FilterTaaArgs* a, LaunchEvents ev, hipStream_t st )
{
	LH2_FLAUNCH( k_filter_unsharpen, filter_grid( a->w, a->h ), dim3( FILTER_TX, FILTER_TY ), st, ev, *a );
}
}
