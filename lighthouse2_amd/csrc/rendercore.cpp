/* rendercore.cpp - host driver of the MI355X wavefront path tracer.

   Counterpart of RenderCore_OptixPrime_B/rendercore.cpp (method-for-method, same semantics),
   re-designed for MI355X:
     - the acceleration structure is our own binned-SAH BVH2 (bvh_build.cpp) instead of the
       closed OptiX Prime BLAS/TLAS (core_mesh.cpp:53-66, rendercore.cpp:250-270);
     - path / ray / hit buffers are SoA float4 planes (coalesced 16-B lane accesses);
     - per-bounce path counts stay on the device (wave-compacted counters), so a frame is one
       stream of launches with no blocking counter copy per bounce (rendercore.cpp:547);
     - shadow rays never overflow (<= 2 per path with ENOUGH_BOUNCES = S_BOUNCED) and are traced
       once per frame with finalizeConnection fused into the any-hit kernel.
*/
#include "rendercore.h"

#include <hip/hip_gl_interop.h>

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "../../include/lh2_detmath.h"
#include "lh2_device.h"

namespace lh2 {

void FatalError( const char* fmt, ... )
{
	char buf[1024];
	va_list args;
	va_start( args, fmt );
	vsnprintf( buf, sizeof( buf ), fmt, args );
	va_end( args );
	throw std::runtime_error( buf );
}

static std::string LibraryDir()
{
	Dl_info info;
	if (dladdr( (void*)&LibraryDir, &info ) && info.dli_fname)
	{
		std::string p( info.dli_fname );
		const size_t s = p.find_last_of( '/' );
		return s == std::string::npos ? std::string( "." ) : p.substr( 0, s );
	}
	return ".";
}

/* ------------------------------------------------------------------------------------------ */
void RenderCore::Init()   /* rendercore.cpp:96-143 */
{
	if (initialized) return;
	CHK_HIP( hipGetDevice( &device ) );
	hipDeviceProp_t props;
	CHK_HIP( hipGetDeviceProperties( &props, device ) );
	smCount = props.multiProcessorCount;
	coreStats.SMcount = (uint32_t)smCount;
	coreStats.ccMajor = (uint32_t)props.major, coreStats.ccMinor = (uint32_t)props.minor;
	coreStats.VRAM = (uint32_t)(props.totalGlobalMem >> 20);
	const char* name = props.gcnArchName[0] ? props.gcnArchName : props.name;
	coreStats.deviceName = new char[strlen( name ) + 1];   /* owned (and leaked) by the core: core_api_base.h:33 */
	memcpy( coreStats.deviceName, name, strlen( name ) + 1 );
	/* the core, side and ahead streams at the device's least priority, which on MI355X (range 0 .. -1) is the default level:
	   the high level for the ahead stream or the core stream measured no faster (profiles/r04k_ab.txt, r04l_ab.txt) */
	{
		int least = 0, greatest = 0;
		CHK_HIP( hipDeviceGetStreamPriorityRange( &least, &greatest ) );
		CHK_HIP( hipStreamCreateWithPriority( &stream, hipStreamNonBlocking, least ) );
		CHK_HIP( hipStreamCreateWithPriority( &sideStream, hipStreamNonBlocking, least ) );
		CHK_HIP( hipStreamCreateWithPriority( &aheadStream, hipStreamNonBlocking, least ) );
	}
	/* blue noise sampler tables (rendercore.cpp:125-134), shipped as data/bluenoise.bin */
	std::string path = getenv( "LH2_BLUENOISE" ) ? getenv( "LH2_BLUENOISE" ) : LibraryDir() + "/data/bluenoise.bin";
	FILE* f = fopen( path.c_str(), "rb" );
	if (!f) FatalError( "blue noise table not found: %s", path.c_str() );
	/* +256 zero bytes: tools_shared.h:343 reads past the table for dimensions > 7 at pixel (127,127)
	   (undefined in the reference; defined as 0 here and in the oracle) */
	std::vector<uint8_t> bn( 65536 * 5 + 256, 0 );
	const size_t got = fread( bn.data(), 1, 65536 * 5, f );
	fclose( f );
	if (got != 65536 * 5) FatalError( "blue noise table truncated: %s", path.c_str() );
	dBlueNoise.upload( bn.data(), bn.size(), stream );
	traceBlocksPerCU7 = std::max( 1, std::min( 8, lh2_trace_blocks_per_cu( 7 ) ) );
	traceBlocksPerCU8 = std::max( 1, std::min( 8, lh2_trace_blocks_per_cu( 8 ) ) );
	maxBlocksPerCU = std::max( traceBlocksPerCU7, traceBlocksPerCU8 );
	blocksPerCU = traceWaves == 7 ? traceBlocksPerCU7 : traceBlocksPerCU8;
	packetBlocksPerCU = std::max( 1, std::min( 8, lh2_packet_blocks_per_cu() ) );
	pathBlocksPerCU = std::max( 1, std::min( 8, lh2_path_blocks_per_cu( 3 ) ) );
	pathBlocksPerCU4 = std::max( 1, std::min( 8, lh2_path_blocks_per_cu( 4 ) ) );
	ps.counters.resize( 2 );
	CHK_HIP( hipMemsetAsync( ps.counters.ptr, 0, sizeof( Counters ) * 2, stream ) );
	ps.cursors.resize( 2 * (size_t)LH2_CURSOR_SLOTS * LH2_CURSOR_WORDS );
	CHK_HIP( hipMemsetAsync( ps.cursors.ptr, 0, sizeof( uint32_t ) * 2 * (size_t)LH2_CURSOR_SLOTS * LH2_CURSOR_WORDS, stream ) );
	ps.rayLog.resize( 2 * LH2_RAYLOG );
	CHK_HIP( hipMemsetAsync( ps.rayLog.ptr, 0, sizeof( uint32_t ) * 2 * LH2_RAYLOG, stream ) );
	/* indexed by pathLength; written by advance_bounce (system scope) */
	CHK_HIP( hipHostMalloc( (void**)&ps.activeLog, sizeof( uint32_t ) * (LH2_MAX_BOUNCES + 8), hipHostMallocCoherent ) );
	for (auto& e : ps.evTrace) CHK_HIP( hipEventCreate( &e ) );
	for (auto& e : ps.evShade) CHK_HIP( hipEventCreate( &e ) );
	for (auto& e : ps.evShadowB) CHK_HIP( hipEventCreate( &e ) );
	for (auto& e : ps.evCount) CHK_HIP( hipEventCreate( &e ) );   /* stop events of launches (LaunchEvents) */
	CHK_HIP( hipEventCreate( &ps.evCamera ) );
	CHK_HIP( hipEventCreate( &ps.evShadow ) );
	CHK_HIP( hipEventCreate( &ps.evSide ) );
	CHK_HIP( hipEventCreateWithFlags( &ps.evEarlyEnd, hipEventDisableTiming ) );
	ps.shSnap.resize( 2 * LH2_SEGS * LH2_SEGCOUNT_STRIDE );
	CHK_HIP( hipHostMalloc( (void**)&hostStats, sizeof( FrameStats ), hipHostMallocCoherent ) );   /* written by k_finalize (system scope) */
	memset( hostStats, 0, sizeof( FrameStats ) );
	for (auto& e : evFrame) CHK_HIP( hipEventCreate( &e ) );
	accel.Init( stream, aheadStream );
	CHK_HIP( hipStreamSynchronize( stream ) );
	initialized = true;
}

void RenderCore::SetTarget( uint32_t w, uint32_t h, uint32_t spp )  /* rendercore.cpp:149-209 */
{
	if (spp < 1) spp = 1;
	if ((uint64_t)w * h * spp > (1u << 24)) FatalError( "path index exceeds 24 bits (camera.h:92): %ux%u x %u spp", w, h, spp );
	scrwidth = (int)w, scrheight = (int)h, scrspp = (int)spp;
	sceneVersion++;
	EnsureBuffers();
	CHK_HIP( hipMemsetAsync( accumulator.ptr, 0, sizeof( float4 ) * (size_t)w * h, stream ) );
	CHK_HIP( hipMemsetAsync( delta.ptr, 0, sizeof( float4 ) * 2 * (size_t)w * h, stream ) );
	samplesTaken = 0;
	fl.historyValid = false;   /* the denoise mode starts over */
}

/* display output (interoptexture.cpp:25-71): register the app's GL_RGBA32F texture with HIP once per
   SetTarget; Render copies the finalized frame into it.  Needs the app's GL context to be current,
   as the reference's interop does; ID 0 (headless RenderSystem, tests, bench) skips it. */
void RenderCore::SetInteropTexture( uint32_t glTextureId )
{
	if (glTextureId == glTexture && (glResource || !glTextureId)) return;
	if (glResource) { CHK_HIP( hipStreamSynchronize( stream ) ); (void)hipGraphicsUnregisterResource( glResource ); glResource = nullptr; }
	glTexture = glTextureId;
	if (!glTextureId) return;
	const unsigned GL_TEXTURE_2D_ = 0x0DE1;
	CHK_HIP( hipGraphicsGLRegisterImage( &glResource, glTextureId, GL_TEXTURE_2D_, hipGraphicsRegisterFlagsWriteDiscard ) );
}

/* Packets share one node fetch per wave (scalar loads, one path for 64 rays): a win while the BVH
   and triangles stay in L2 / Infinity Cache, a loss when node fetches go to DRAM, where the
   per-ray loop's 64 independent loads per wave hide latency better (config 2: 8.6 MB, packets
   1.6x faster; 1M-tri room 81 MB: 12 % slower; 10M-tri instanced 1 GB: 1.5x slower;
   profiles/r01b_ab_packets.jsonl) */
bool RenderCore::UsePackets() const
{
	if (packetPrimary >= 0) return packetPrimary != 0;
	return accel.Bytes() <= kPacketMaxBytes;
}

/* traversal loop of the per-ray launches (setting "traceVersion"): 7, the BVH4 loop (lh2_trace4d.inc), unless
   the BVH4 is not built (setting "bvh4" 0) or the reference BVH2 loop is asked for (1) */
int RenderCore::TraceVersion() const { return (traceVersion == 1 || !accel.build.bvh4) ? 1 : 7; }

void RenderCore::EnsureBuffers()
{
	accumulator.resize( (FilterOn() ? 2 : 1) * (size_t)scrwidth * scrheight );   /* the denoise mode: direct and indirect planes */
	frame.resize( (size_t)scrwidth * scrheight );
	delta.resize( 2 * (size_t)scrwidth * scrheight );   /* per frame parity: the next frame's first shade may run beside this finalize */
	if (FilterOn()) EnsureFilterBuffers();
}

/* the denoise mode's buffers, for the current target; a new size starts without history */
void RenderCore::EnsureFilterBuffers()
{
	const size_t n = (size_t)scrwidth * scrheight;
	if (!fl.ev[0]) for (auto& e : fl.ev) CHK_HIP( hipEventCreate( &e ) );
	if (!n) return;
	if (fl.pixels != n)
	{
		fl.features.resize( n ), fl.deltaDepth.resize( n ), fl.shading.resize( n ), fl.motion.resize( n );
		for (int i = 0; i < 2; i++) fl.worldPos[i].resize( n ), fl.moments[i].resize( n ), fl.filtered[i].resize( n );
		/* the history counts start at 0, and no record is read before it was written */
		CHK_HIP( hipMemsetAsync( fl.features.ptr, 0, sizeof( uint4 ) * n, stream ) );
		for (int i = 0; i < 2; i++)
		{
			CHK_HIP( hipMemsetAsync( fl.worldPos[i].ptr, 0, sizeof( float4 ) * n, stream ) );
			CHK_HIP( hipMemsetAsync( fl.moments[i].ptr, 0, sizeof( float4 ) * n, stream ) );
			CHK_HIP( hipMemsetAsync( fl.filtered[i].ptr, 0, sizeof( float4 ) * n, stream ) );
		}
		fl.pixels = n, fl.historyValid = false, fl.cur = 0;
	}
	EnsureTaaBuffers();
}

/* the TAA stage's buffers (setting "TAA"), beside the filter's and of their size, only while both settings are applied;
   new ones start without TAA history */
void RenderCore::EnsureTaaBuffers()
{
	const size_t n = fl.pixels;
	if (!TaaOn() || !n || fl.taaPixels == n) return;
	fl.linear.resize( n ), fl.taa[0].resize( n ), fl.taa[1].resize( n );
	CHK_HIP( hipMemsetAsync( fl.linear.ptr, 0, sizeof( float4 ) * n, stream ) );
	for (int i = 0; i < 2; i++) CHK_HIP( hipMemsetAsync( fl.taa[i].ptr, 0, sizeof( float4 ) * n, stream ) );
	fl.taaPixels = n, fl.taaValid = false;
}
void RenderCore::FreeTaaBuffers()
{
	fl.linear.free(), fl.taa[0].free(), fl.taa[1].free();
	fl.taaPixels = 0, fl.taaValid = false;
}

/* the denoise mode allowed or not (MultiDevice): as if the setting "filter" changed */
void RenderCore::SetFilterAllowed( bool on )
{
	if (on == filterAllowed) return;
	const bool want = filterOn;
	Setting( "filter", 0.0f );   /* off under the old permission: frees the buffers if it was on */
	filterAllowed = on;
	Setting( "filter", want ? 1.0f : 0.0f );
}

/* path buffers for `paths` paths (a bit extra, as the reference reserves, and room for LH2_SEGS segments
   of ceil(paths / LH2_SEGS)); shadow rays: 2 per path */
void RenderCore::EnsurePaths( uint32_t paths )
{
	if (!PathsFit( paths ))
	{
		ps.cap = (size_t)paths + (paths >> 4) + 64;
		for (int i = 0; i < 2; i++) ps.rayO[i].resize( ps.cap ), ps.rayD[i].resize( ps.cap ), ps.T4[i].resize( ps.cap ), ps.Q4[i].resize( ps.cap );
		ps.hits.resize( ps.cap );
		for (int i = 0; i < 2; i++) ps.rayOP[i].resize( ps.cap ), ps.rayDP[i].resize( ps.cap ), ps.T4P[i].resize( ps.cap ), ps.Q4P[i].resize( ps.cap ), ps.hitsP[i].resize( ps.cap );
		ps.relaid = true;
		/* shadow rays: 2 per path, per frame parity */
		ps.shCap = 2 * ps.cap, ps.shMaskWords = (ps.shCap + 63) / 32 + 2;
		ps.shO.resize( 2 * ps.shCap ), ps.shD.resize( 2 * ps.shCap ), ps.shP.resize( 2 * ps.shCap );
		ps.shMask.resize( 2 * ps.shMaskWords );
	}
	EnsureStack();
}

void RenderCore::EnsureStack()
{
	/* sized for the largest grid traceBlocksPerCU / traceWaves may select later */
	const size_t need = (size_t)(LH2_STACK_TOTAL - LH2_STACK_LDS) * smCount * maxBlocksPerCU * 256;
	if (ps.gstack.count < need) ps.gstack.resize( need );
	if (shadowOverlap && ps.sideStack.count < need) ps.sideStack.resize( need );
	if (cameraFused && kCamAhead && ps.aheadStack.count < need) ps.aheadStack.resize( need );
}

void RenderCore::Setting( const char* name, float value )  /* rendercore.cpp:439-457 */
{
	if (!strcmp( name, "epsilon" )) geometryEpsilon = value;
	else if (!strcmp( name, "clampValue" )) clampValue = value;
	else if (!strcmp( name, "maxPathLength" )) maxPathLength = std::min( 16, std::max( 1, (int)value ) );
	/* PrimeRef validation mode: the RenderCore_PrimeRef path tracer (uniform random numbers, Lambert
	   BSDF, NEE without MIS, Russian roulette, MAXPATHLENGTH 64) on the same scene data */
	else if (!strcmp( name, "primeRef" )) primeRef = value != 0;
	else if (!strcmp( name, "tiledRays" )) tiledRays = value != 0;
	/* dynamic ray fetch: refill a wave's idle lanes once this many are idle (64 = whole batches);
	   coherent 8x8-tiled primary rays trace best in batches, incoherent bounce rays with refills */
	else if (!strcmp( name, "refill" )) refillOther = std::min( 64, std::max( 1, (int)value ) );
	/* traversal: test parked BLAS leaves once this many lanes of a wave hold one (0 = every step) */
	else if (!strcmp( name, "leafBatch" )) leafBatch = std::min( 64, std::max( 0, (int)value ) );
	/* BLAS build parameters, used by later SetGeometry calls */
	else if (!strcmp( name, "bvhMaxLeaf" )) accel.build.maxLeaf = std::min( 16, std::max( 1, (int)value ) );
	else if (!strcmp( name, "bvhSpatial" )) accel.build.spatial = std::max( 0.0f, value );   /* SBVH overlap threshold (x root area); 0: off */
	else if (!strcmp( name, "bvhSpatialBudget" )) accel.build.spatialBudget = std::min( 4.0f, std::max( 0.0f, value ) );
	else if (!strcmp( name, "bvhSpatialMinRefs" )) accel.build.spatialMinRefs = std::max( 0, (int)value );
	else if (!strcmp( name, "bvh4Collapse" )) accel.build.bvh4Collapse = value != 0;
	else if (!strcmp( name, "bvh4" )) accel.build.bvh4 = value != 0;   /* before SetGeometry */
	else if (!strcmp( name, "gpuBuild" )) accel.gpuBuild = value != 0;          /* BLAS builder of later SetGeometry calls */
	else if (!strcmp( name, "buildThreads" )) accel.buildThreads = std::max( 0, (int)value );   /* host threads of the deferred CPU builds */
	else if (!strcmp( name, "gpuTlas" )) { accel.gpuTlas = value != 0; accel.InstancesChanged(); }
	else if (!strcmp( name, "chordSplit" )) chordSplit = std::max( 0.0f, value );   /* two-ended path segments (longest first); 0: off */
	else if (!strcmp( name, "packetHeavy" )) packetHeavy = value < 0 ? -1.0f : value;   /* heavy-first primary packets; 0: off; -1: by frame */
	else if (!strcmp( name, "pathTail" )) pathTail = std::max( 0, (int)value );   /* bounces from this one in one trace-and-shade launch; 0: off */
	else if (!strcmp( name, "pathTailBatch" )) pathTailBatch = std::min( 64, std::max( 1, (int)value ) );
	else if (!strcmp( name, "shadowOverlap" )) shadowOverlap = value != 0;
	else if (!strcmp( name, "cameraFused" )) cameraFused = value != 0;
	else if (!strcmp( name, "frameOverlap" )) frameOverlap = (int)value;
	else if (!strcmp( name, "earlyShade" )) earlyShade = value != 0;
	else if (!strcmp( name, "sideBlocks" )) sideBlocks = std::min( 8, std::max( -1, (int)value ) );
	else if (!strcmp( name, "pathTailBlocks" )) pathTailBlocks = std::min( 8, std::max( 0, (int)value ) );
	else if (!strcmp( name, "shadeBlocks" )) shadeBlocks = std::min( 64, std::max( 0, (int)value ) );
	else if (!strcmp( name, "finalShadowBlocks" )) finalShadowBlocks = std::min( 8, std::max( 0, (int)value ) );
	else if (!strcmp( name, "pathTailWaves" )) pathTailWaves = std::min( 4, std::max( 0, (int)value ) );
	/* packet traversal of tiled primary rays: 1 on, 0 off, -1 when the BVH + triangles fit in packetMaxMB */
	else if (!strcmp( name, "packetPrimary" )) packetPrimary = value < 0 ? -1 : value != 0;
	else if (!strcmp( name, "singleInstanceStart" )) singleInstanceStart = value != 0;   /* one instance: rays start at its TLAS leaf */
	else if (!strcmp( name, "terminalShade" )) terminalShade = value != 0;   /* drop hits that cannot contribute before shading them (ShadeParams::terminal) */
	else if (!strcmp( name, "traceBlocksPerCU" ))   /* persistent trace grid: blocks per CU (0: the launched variant's occupancy) */
	{
		userBlocksPerCU = value > 0 ? std::min( maxBlocksPerCU, std::max( 1, (int)value ) ) : 0;
		blocksPerCU = userBlocksPerCU ? userBlocksPerCU : traceWaves == 7 ? traceBlocksPerCU7 : traceBlocksPerCU8;
	}
	else if (!strcmp( name, "unitTraceWaves" )) unitTraceWaves = (int)value == 8 ? 8 : 7;   /* the same for the unit queries (TraceClosest*) */
	else if (!strcmp( name, "traceWaves" ))   /* closest-hit kernel variant (7 or 8 waves per SIMD; 0: by scene); resets traceBlocksPerCU */
	{
		traceWaves = (int)value == 7 ? 7 : (int)value == 8 ? 8 : 0;
		userBlocksPerCU = 0;
		blocksPerCU = traceWaves == 7 ? traceBlocksPerCU7 : traceBlocksPerCU8;
	}
	else if (!strcmp( name, "unitCoherent" )) unitCoherent = value != 0;   /* TraceClosestDevice traces as the frame traces primary rays */
	else if (!strcmp( name, "traceVersion" )) traceVersion = (int)value == 1 ? 1 : 0;   /* 1: the reference BVH2 loop; else the BVH4 loop */
	/* the denoise mode (SVGF: lh2_filter.h): every Render delivers a filtered frame of that frame's samples and the
	   reprojected history; the light clamps are those of its prepare step */
	else if (!strcmp( name, "filter" ))
	{
		const bool was = FilterOn();
		filterOn = value != 0;
		const bool now = FilterOn();
		if (was != now && initialized)
		{
			/* the frames in flight end; the accumulator gets or loses its second plane, the filter's buffers come or go, and
			   the next frame starts the accumulation over */
			CHK_HIP( hipStreamSynchronize( aheadStream ) );
			CHK_HIP( hipStreamSynchronize( sideStream ) );
			CHK_HIP( hipStreamSynchronize( stream ) );
			if (!now)
			{
				fl.features.free(), fl.deltaDepth.free(), fl.shading.free(), fl.motion.free();
				for (int i = 0; i < 2; i++) fl.worldPos[i].free(), fl.moments[i].free(), fl.filtered[i].free();
				fl.pixels = 0, fl.historyValid = false;
				FreeTaaBuffers();
			}
			if (scrwidth)
			{
				accumulator.free();
				EnsureBuffers();
				CHK_HIP( hipMemsetAsync( accumulator.ptr, 0, sizeof( float4 ) * accumulator.count, stream ) );
				sceneVersion++;
			}
			samplesTaken = 0, firstConvergingFrame = true;
		}
	}
	else if (!strcmp( name, "clampDirect" )) clampDirect = value;
	else if (!strcmp( name, "clampIndirect" )) clampIndirect = value;
	/* the a-trous passes' taps: 1 from an LDS tile, 0 through L1 / L2, -1 the measured pick per pass (RunFilter) */
	else if (!strcmp( name, "filterLds" )) filterLds = value < 0 ? -1 : value != 0;
	/* temporal antialiasing as the end of the filter chain (k_filter_taa, k_filter_unsharpen): applied only where the filter
	   is (TaaOn); the wish is kept while it is not.  A RenderSystem host sends it before every frame */
	else if (!strcmp( name, "TAA" ))
	{
		if ((value != 0) == taaOn) return;
		const bool was = TaaOn();
		taaOn = value != 0;
		if (was != TaaOn() && initialized)
		{
			/* the frames in flight end; the stage's buffers come or go and it starts without history of its own.  The filter's
			   history and the sample count stay */
			CHK_HIP( hipStreamSynchronize( aheadStream ) );
			CHK_HIP( hipStreamSynchronize( sideStream ) );
			CHK_HIP( hipStreamSynchronize( stream ) );
			if (was) FreeTaaBuffers(); else EnsureTaaBuffers();
		}
	}
	/* other names are ignored, as in the reference */
}

/* the current value of a setting (extension: the reference has no getter); false for unknown names */
bool RenderCore::GetSetting( const char* name, float& value ) const
{
	const BuildSettings& bs = accel.build;
	struct { const char* n; float v; } t[] = {
		{ "epsilon", geometryEpsilon }, { "clampValue", clampValue }, { "maxPathLength", (float)maxPathLength },
		{ "primeRef", (float)primeRef }, { "tiledRays", (float)tiledRays }, { "refill", (float)refillOther }, { "leafBatch", (float)leafBatch },
		{ "bvhMaxLeaf", (float)bs.maxLeaf }, { "bvhSpatial", bs.spatial }, { "bvhSpatialBudget", bs.spatialBudget }, { "bvhSpatialMinRefs", (float)bs.spatialMinRefs },
		{ "bvh4Collapse", (float)bs.bvh4Collapse }, { "bvh4", (float)bs.bvh4 }, { "gpuBuild", (float)accel.gpuBuild }, { "buildThreads", (float)accel.buildThreads }, { "gpuTlas", (float)accel.gpuTlas },
		{ "chordSplit", chordSplit }, { "packetHeavy", packetHeavy }, { "pathTail", (float)pathTail }, { "pathTailBatch", (float)pathTailBatch },
		{ "shadowOverlap", (float)shadowOverlap }, { "cameraFused", (float)cameraFused }, { "frameOverlap", (float)frameOverlap }, { "earlyShade", (float)earlyShade },
		{ "sideBlocks", (float)sideBlocks }, { "pathTailBlocks", (float)pathTailBlocks }, { "shadeBlocks", (float)shadeBlocks }, { "finalShadowBlocks", (float)finalShadowBlocks },
		{ "pathTailWaves", (float)pathTailWaves }, { "packetPrimary", (float)packetPrimary }, { "singleInstanceStart", (float)singleInstanceStart },
		{ "terminalShade", (float)terminalShade }, { "traceBlocksPerCU", (float)ClosestBlocksPerCU( ScenePicksWaves() ) }, { "unitTraceWaves", (float)unitTraceWaves }, { "traceWaves", (float)traceWaves },
		{ "unitCoherent", (float)unitCoherent }, { "traceVersion", (float)TraceVersion() },
		{ "usePackets", (float)UsePackets() }, { "blasBuilds", (float)BlasBuildCount() },
		{ "filter", (float)FilterOn() }, { "clampDirect", clampDirect }, { "clampIndirect", clampIndirect }, { "filterLds", (float)filterLds },
		{ "TAA", (float)TaaOn() } };
	for (const auto& e : t) if (!strcmp( name, e.n )) { value = e.v; return true; }
	return false;
}

void RenderCore::SetTextures( const lh2_CoreTexDesc* tex, int textureCount )   /* rendercore.cpp:276-292 */
{
	sceneVersion++;   /* device-resident scene data: the next fused frame's primary launch waits for the previous frame */
	texDescs.assign( tex, tex + std::max( 0, textureCount ) );
	/* SyncStorageType (rendercore.cpp:299-336) for ARGB32, ARGB128 and NRM32: one continuous array per
	   storage type, textures in descriptor order, at least 16 texels.  ARGB128 texels are copied whole
	   (the reference copies pixelCount * 4 bytes of each 16-byte texel there; this core never reads
	   ARGB128 texels while shading, so only CoreStats sees the difference). */
	for (int storage = 0; storage < 3; storage++)
	{
		uint32_t total = 0;
		for (auto& t : texDescs) if (t.storage == storage) total += t.pixelCount;
		const uint32_t alloc = std::max( 16u, total );
		if (storage == 1)
		{
			std::vector<float4> buf( alloc, make_float4( 0, 0, 0, 0 ) );
			uint32_t at = 0;
			for (auto& t : texDescs) if (t.storage == storage) { memcpy( buf.data() + at, t.idata, (size_t)t.pixelCount * 16 ); t.firstPixel = at; at += t.pixelCount; }
			dArgb128.upload( buf.data(), buf.size(), stream );
			coreStats.argb128TexelCount = alloc;
		}
		else
		{
			std::vector<uint32_t> buf( alloc, 0u );
			uint32_t at = 0;
			for (auto& t : texDescs) if (t.storage == storage) { memcpy( buf.data() + at, t.idata, (size_t)t.pixelCount * 4 ); t.firstPixel = at; at += t.pixelCount; }
			(storage == 0 ? dArgb32 : dNrm32).upload( buf.data(), buf.size(), stream );
			(storage == 0 ? coreStats.argb32TexelCount : coreStats.nrm32TexelCount) = alloc;
		}
	}
	CHK_HIP( hipStreamSynchronize( stream ) );   /* texel pointers are borrowed for this call only */
}

#define TOCHAR(a) lh2_f2u( (a) * 255.0f )
#define TOUINT4(a,b,c,d) (TOCHAR(a)+(TOCHAR(b)<<8)+(TOCHAR(c)<<16)+(TOCHAR(d)<<24))
void RenderCore::SetMaterials( const lh2_CoreMaterial* mat, int n )   /* rendercore.cpp:353-399 */
{
	sceneVersion++;   /* device-resident scene data: the next fused frame's primary launch waits for the previous frame */
	std::vector<uint4> recs( (size_t)std::max( n, 1 ) * 8 );
	memset( recs.data(), 0, recs.size() * sizeof( uint4 ) );
	diffuseOnly = true, canEmit = false;
	for (int i = 0; i < n; i++)
	{
		const lh2_CoreMaterial& m = mat[i];
		/* IsEmissive (colour > 1 after the fp16 round, which keeps x <= 1 at or below 1; NaN counts as
		   emissive here), colour and detail maps (texels can exceed 1) and alpha cut-outs */
		if (!(m.color.value.x <= 1.0f && m.color.value.y <= 1.0f && m.color.value.z <= 1.0f) || m.color.textureID != -1 ||
			m.detailColor.textureID != -1 || (m.flags & 2))
			canEmit = true;
		/* a path can only continue past its second vertex through a specular event (ROUGHNESS <= 0.001,
		   a transmission sample) or an alpha cut-out (ENOUGH_BOUNCES = S_BOUNCED, pathtracer.h:33,211) */
		if (TOCHAR( m.roughness.value ) == 0 || TOCHAR( m.transmission.value ) != 0 || (m.flags & 2) || m.roughness.textureID != -1)
			diffuseOnly = false;
		const uint32_t r = lh2_f2h( m.color.value.x ), g = lh2_f2h( m.color.value.y ), b = lh2_f2h( m.color.value.z );
		const uint32_t tr = lh2_f2h( 1 - m.absorption.value.x ), tg = lh2_f2h( 1 - m.absorption.value.y ), tb = lh2_f2h( 1 - m.absorption.value.z );
		const uint32_t flags = (m.eta.value < 1 ? 1u : 0u) + ((m.flags & 1) ? (1u << 11) : 0u) + ((m.flags & 2) ? (1u << 12) : 0u);
		recs[i * 8 + 0] = make_uint4( r | (g << 16), b | (tr << 16), tg | (tb << 16), flags );
		recs[i * 8 + 1] = make_uint4( TOUINT4( m.metallic.value, m.subsurface.value, m.specular.value, m.roughness.value ),
			TOUINT4( m.specularTint.value, m.anisotropic.value, m.sheen.value, m.sheenTint.value ),
			TOUINT4( m.clearcoat.value, m.clearcoatGloss.value, m.transmission.value, 0 ), lh2_f2b( m.eta.value ) );
		/* texture / normal map records (rendercore.cpp:379-384, RenderCore::Map rendercore.h:79-86):
		   x = width | height << 16 (shorts), y / z = uvscale / uvoffset (halves), w = first texel */
		auto map = [&]( int tid, lh2_float2 uvscale, lh2_float2 uvoffs ) {
			if (tid < 0 || tid >= (int)texDescs.size()) FatalError( "SetMaterials: material %d uses texture %d of %d (call SetTextures first)", i, tid, (int)texDescs.size() );
			const lh2_CoreTexDesc& t = texDescs[tid];
			return make_uint4( (t.width & 0xffffu) | ((t.height & 0xffffu) << 16), lh2_f2h( uvscale.x ) | ((uint32_t)lh2_f2h( uvscale.y ) << 16),
				lh2_f2h( uvoffs.x ) | ((uint32_t)lh2_f2h( uvoffs.y ) << 16), t.firstPixel );
		};
		uint32_t texFlags = 0;
		if (m.color.textureID != -1) recs[i * 8 + 2] = map( m.color.textureID, m.color.uvscale, m.color.uvoffset ), texFlags |= 1u << 2;
		if (m.detailColor.textureID != -1) recs[i * 8 + 3] = map( m.detailColor.textureID, m.detailColor.uvscale, m.detailColor.uvoffset ), texFlags |= 1u << 9;
		if (m.normals.textureID != -1) recs[i * 8 + 4] = map( m.normals.textureID, m.normals.uvscale, m.normals.uvoffset ), texFlags |= 1u << 3;
		if (m.detailNormals.textureID != -1) recs[i * 8 + 5] = map( m.detailNormals.textureID, m.detailNormals.uvscale, m.detailNormals.uvoffset ), texFlags |= 1u << 7;
		if (m.specular.textureID != -1) recs[i * 8 + 6] = map( m.specular.textureID, m.specular.uvscale, m.specular.uvoffset ), texFlags |= 1u << 4;
		if (m.roughness.textureID != -1) recs[i * 8 + 7] = map( m.roughness.textureID, m.roughness.uvscale, m.roughness.uvoffset ), texFlags |= 1u << 5;
		/* DIFFUSEMAPISHDR: the reference tests textureID != 1 and so reads texDescs[-1] for untextured
		   materials (rendercore.cpp:386); here only a valid diffuse map can set it.  Not read by shading. */
		if (m.color.textureID >= 0 && (texDescs[m.color.textureID].flags & 8)) texFlags |= 1u << 1;
		recs[i * 8 + 0].w |= texFlags;
	}
	dMaterials.upload( recs.data(), recs.size(), stream );
	materialCount = n;
	CHK_HIP( hipStreamSynchronize( stream ) );
}

void RenderCore::SetLights( const lh2_CoreLightTri* a, int na, const lh2_CorePointLight* p, int np, const lh2_CoreSpotLight* s, int ns,
	const lh2_CoreDirectionalLight* d, int nd )   /* rendercore.cpp:405-419 */
{
	sceneVersion++;
	dArea.upload( a, na, stream ), dPoint.upload( p, np, stream ), dSpot.upload( s, ns, stream ), dDir.upload( d, nd, stream );
	dArea.resize( 1 ), dPoint.resize( 1 ), dSpot.resize( 1 ), dDir.resize( 1 );
	nArea = na, nPoint = np, nSpot = ns, nDir = nd;
	CHK_HIP( hipStreamSynchronize( stream ) );
}

void RenderCore::SetSkyData( const float* pixels, uint32_t width, uint32_t height )   /* rendercore.cpp:425-433 */
{
	sceneVersion++;   /* device-resident scene data: the next fused frame's primary launch waits for the previous frame */
	dSky.upload( pixels, (size_t)width * height * 3, stream );
	dSky.resize( 1 );
	skyW = (int)width, skyH = (int)height;
	CHK_HIP( hipStreamSynchronize( stream ) );
}

/* the scene calls go to the SceneAccel (scene_accel.cpp); what stays here is sceneVersion: new device-resident scene data,
   so the next fused frame's primary launch waits for the previous frame.  An instance-only UpdateToplevel leaves it alone
   (it writes the TLAS slot no frame in flight reads), so the next frame may still overlap */
void RenderCore::SetGeometry( int meshIdx, const float*, int, int triangleCount, const lh2_CoreTri* tris, const uint32_t* )
{
	sceneVersion++;
	accel.SetGeometry( meshIdx, triangleCount, tris );
}
void RenderCore::AdoptGeometry( int meshIdx, int triangleCount, const lh2_CoreTri* tris, const RenderCore& src )
{
	sceneVersion++;
	accel.AdoptGeometry( meshIdx, triangleCount, tris, src.accel );
}
void RenderCore::UpdateToplevel() { if (accel.UpdateToplevel()) sceneVersion++; }

#ifdef LH2_TOUCH
/* the unique records one closest-hit launch reads (diagnostic build): quantized BVH4 nodes (64 B) and leaf triangle records
   (48 B), one bit each, counted after the launch; one JSON line per launch on stderr.  The launch is serialised with the
   count (the build is for this count, not for timing) */
void RenderCore::TouchBegin()
{
	CHK_HIP( hipDeviceSynchronize() );   /* nothing in flight reads the bitmap pointer while it changes */
	const uint32_t nodeWords = accel.TouchNodeWords(), triWords = accel.TouchTriWords();
	touchMap.resize( (size_t)nodeWords + triWords );
	CHK_HIP( hipMemsetAsync( touchMap.ptr, 0, sizeof( uint32_t ) * ((size_t)nodeWords + triWords), stream ) );
	lh2_touch_set( touchMap.ptr, nodeWords, nodeWords + triWords );
	touchNodeWords = nodeWords;
}
void RenderCore::TouchReport( int pathLength )
{
	CHK_HIP( hipDeviceSynchronize() );
	std::vector<uint32_t> h( touchMap.count );
	CHK_HIP( hipMemcpy( h.data(), touchMap.ptr, sizeof( uint32_t ) * h.size(), hipMemcpyDeviceToHost ) );
	uint64_t nodes = 0, tris = 0;
	for (size_t i = 0; i < h.size(); i++) (i < touchNodeWords ? nodes : tris) += (uint64_t)__builtin_popcount( h[i] );
	fprintf( stderr, "LH2_TOUCH {\"pathLength\": %d, \"unique_nodes\": %llu, \"unique_tri_records\": %llu, \"node_bytes\": %llu, "
		"\"tri_bytes\": %llu, \"scene_nodes\": %d, \"scene_tri_records\": %d, \"paths\": %u}\n", pathLength, (unsigned long long)nodes,
		(unsigned long long)tris, (unsigned long long)nodes * 64ull, (unsigned long long)tris * 48ull, accel.Node4Count(), accel.TriRecordCount(), ps.count );
	lh2_touch_set( nullptr, 0, 0 );   /* later closest-hit launches (unit queries) record nothing */
}
#endif

/* device-side scene errors (TLAS deeper than the traversal stack): the trace kernels skip the
   frame, and the host reports it here */
#define LH2_STR_( x ) #x
#define LH2_XSTR( x ) LH2_STR_( x )
static const char* SceneErrorText( int e )
{
	if (e & LH2_SCENE_ERR_QRANGE) return "scene extent beyond the quantized BVH4 grid (a node wider than 255 * 2^27 or coordinates beyond 2^55)";
	return "BVH depth exceeds the traversal stack (" LH2_XSTR( LH2_STACK_TOTAL ) " levels)";
}

void RenderCore::CheckSceneError()
{
	const int* err = accel.SceneErr( accel.Slot() );
	if (!err) return;
	int e = 0;
	accel.SyncTlas();
	CHK_HIP( hipMemcpyAsync( &hostStats->sceneError, err, sizeof( int ), hipMemcpyDeviceToHost, stream ) );
	CHK_HIP( hipStreamSynchronize( stream ) );
	e = hostStats->sceneError;
	if (e) FatalError( "%s", SceneErrorText( e ) );
}

SceneDev RenderCore::MakeSceneDev()
{
	SceneDev s;
	accel.Fill( s, singleInstanceStart );
	s.argb32 = dArgb32.ptr, s.nrm32 = dNrm32.ptr;
	s.argb32Count = (uint32_t)dArgb32.count, s.nrm32Count = (uint32_t)dNrm32.count;
	s.materials = dMaterials.ptr;
	s.areaLights = dArea.ptr, s.pointLights = dPoint.ptr, s.spotLights = dSpot.ptr, s.dirLights = dDir.ptr;
	s.nArea = nArea, s.nPoint = nPoint, s.nSpot = nSpot, s.nDir = nDir;
	s.sky = dSky.ptr, s.skyW = skyW, s.skyH = skyH;
	s.blueNoise = dBlueNoise.ptr;
	s.geometryEpsilon = geometryEpsilon, s.clampValue = clampValue;
	return s;
}

static inline uint32_t XorShift( uint32_t& s ) { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; }  /* platform/system.cpp:48 */

/* the view's camera basis: right = p2 - p1, up = p3 - p1 */
static void SetCameraView( CameraParams& cp, const lh2_ViewPyramid& view )
{
	cp.pos = view.pos, cp.p1 = view.p1;
	cp.right = { view.p2.x - view.p1.x, view.p2.y - view.p1.y, view.p2.z - view.p1.z };
	cp.up = { view.p3.x - view.p1.x, view.p3.y - view.p1.y, view.p3.z - view.p1.z };
}

/* a frame being queued: its plan, and what Render's stages hand on to each other */
struct Frame
{
	const FramePlan plan;
	const lh2_ViewPyramid& view;
	SceneDev sd{};
	int tlas = 0;                        /* the TLAS slot this frame reads (released after its finalize) */
	FrameSlots s{};                      /* this frame's parity: its counters, work-queue heads, shadow stream and ray-count log */
	CameraParams cp{};
	int in = 0;                          /* the ping-pong set the bounce reads; its shade launch writes the other one */
	int pl = 0, tailL = 0;               /* bounces launched so far; the path-tail launch, once queued */
	bool snapped = false, sideOn = false;   /* the shadow rays before the tail: snapshot taken, traced on the side stream */
	uint32_t* hvReadBlock = nullptr;     /* the heavy-packet block the primary packets read */
};

FrameSlots RenderCore::Slots() const
{
	const size_t fp = (size_t)ps.fp;
	return { ps.counters.ptr + fp, ps.cursors.ptr + fp * LH2_CURSOR_SLOTS * LH2_CURSOR_WORDS, ps.rayLog.ptr + fp * LH2_RAYLOG,
		ps.shO.ptr + fp * ps.shCap, ps.shD.ptr + fp * ps.shCap, ps.shP.ptr + fp * ps.shCap,
		ps.shMask.ptr + fp * ps.shMaskWords, ps.shSnap.ptr + fp * LH2_SEGS * LH2_SEGCOUNT_STRIDE, delta.ptr + fp * scrwidth * scrheight };
}

/* a frame is six steps: the plan (every decision, no HIP call), the state transitions and buffers, then the launch stages.
   CoreStats timings come from the stop events recorded by the launches themselves (LaunchEvents): no hipEventRecord
   between kernels */
void RenderCore::Render( const lh2_ViewPyramid& view, int converge )   /* rendercore.cpp:463-609 */
{
	if (!initialized) FatalError( "Render before Init" );
	if (!scrwidth) FatalError( "Render before SetTarget" );
	if (accel.Dirty()) UpdateToplevel();
	if (!dMaterials.ptr) FatalError( "Render before SetMaterials" );
	const auto t0 = std::chrono::high_resolution_clock::now();
	Frame f{ PlanFrame( view, converge ), view };
	BeginFrame( f, converge );
	PrimaryStage( f );
	BounceLoop( f );
	FinalShadows( f );
	FinishFrame( f );
	frameHostMs = std::chrono::duration<double, std::milli>( std::chrono::high_resolution_clock::now() - t0 ).count();
}

/* every decision of the frame, from the settings, the scene facts and the state that crosses frames (PathStreams); a mode
   (the filter, PrimeRef) appears here, not in the stages */
FramePlan RenderCore::PlanFrame( const lh2_ViewPyramid& view, int converge ) const
{
	FramePlan p{};
	p.restart = converge == LH2_RESTART || firstConvergingFrame;
	p.tileRows = TileRows();
	p.pathCount = (uint32_t)p.tileRows * (uint32_t)scrwidth * (uint32_t)scrspp;
	/* segmented path / ray streams (lh2_kernels.h): LH2_SEGS segments of segStride records */
	p.segStride = (p.pathCount + LH2_SEGS - 1) / LH2_SEGS;
	p.small = (float)p.pathCount <= kSmallFramePaths;
	/* the denoise mode (whole frames only: a tile has no neighbours across its edge; not in PrimeRef mode): the plain
	   wavefront loop, one launch pair per bounce behind the previous frame - no path tail, no early or terminal shade, no
	   overlap of consecutive frames; the accumulator (two planes) holds this frame's samples only, and the lens is a pinhole */
	p.filt = FilterOn() && fl.pixels && p.tileRows == scrheight && !primeRef;
	p.taa = p.filt && TaaOn() && fl.taaPixels;
	p.aperture = p.filt ? 0.0f : view.aperture;
	p.packets = tiledRays && UsePackets();
	/* heavy-first primary packets: this frame reads the block the previous one recorded, and records into the
	   other one (a new layout, hvRelayout, zeroes both) */
	p.hvOn = packetHeavy != 0 && p.packets && !primeRef;
	p.hvCap = (p.segStride + 63) / 64;
	p.hvRelayout = p.hvOn && p.hvCap != ps.hvCap;
	for (int k = 0; k < LH2_SEGS; k++)
	{
		const uint32_t lo = (uint32_t)k * p.segStride, n = p.pathCount > lo ? std::min( p.pathCount - lo, p.segStride ) : 0u;
		p.hvTiles += (n + 63) / 64;
	}
	p.growPaths = !PathsFit( p.pathCount );
	p.traceGrid = TraceGrid();
	/* the shade launches walk their segment with a static block stride: blocks beyond the resident ones start as others
	   end, so more, smaller block shares balance the launch's end.  shadeBlocks 0: about shadePathsPerThread paths per
	   thread, between the trace grid and shadeMaxBlocks per CU (the N = 8 share 12 per CU, config 3 24: -1.5 / -1.5 %,
	   profiles/r04al_ab.txt, r04am_ab.txt) */
	p.shadeGrid = shadeBlocks > 0 ? smCount * shadeBlocks : std::max( p.traceGrid, std::min( smCount * kShadeMaxBlocks,
		(int)((double)p.pathCount / (256.0 * kShadePathsPerThread)) ) );
	/* the camera fused into the primary packet launch: the heavy-packet block it records into must be zero (the previous
	   fused frame's first shade launch zeroed it) */
	p.fusedCam = cameraFused && p.packets && !primeRef;
	/* round 6: a frame whose primary rays are traced per ray (no packets: a scene beyond the Infinity Cache,
	   config 5) takes the same frame overlap.  Its camera launch (with the frame's resets) and its per-ray primary launch
	   write the frame parity's primary buffers on the ahead stream, the primary launch with a global stack of its own
	   (PathStreams::aheadStack: the previous frame's bounce launch still uses gstack) */
	p.camAhead = kCamAhead && !p.fusedCam && cameraFused && !primeRef && TraceVersion() == 7;
	p.pFrame = p.fusedCam || p.camAhead;   /* the frame's primary stage may run beside the previous frame */
	/* the primary stage beside the previous frame (frame overlap), or behind it on the core stream: on a restart (the
	   launch zeroes accumulator pixels), after a change of scene data, buffers (BeginFrame is about to grow them) or tile,
	   or when the previous frame had no such primary stage */
	const bool relaid = ps.relaid || p.growPaths || p.hvRelayout;
	p.serialize = p.filt || !frameOverlap || !ps.lastFused || relaid || tileChanged || sceneVersion != ps.lastSceneVersion;
	/* the accumulator reset of a restart is folded into the camera launch (each pixel's first sample zeroes it; rows outside
	   this rank's tile stay zero from SetTarget); a changed tile clears the whole frame.  A restart beside the previous
	   frame: the accumulator is zeroed on the core stream, behind the previous frame's finalize and before this frame's
	   first addition there (the early shade adds into the delta), not by the primary launch */
	p.clearAll = p.restart && tileChanged;
	p.clearBehind = p.restart && !tileChanged && !p.filt && p.pFrame && !p.serialize;
	p.clearByLaunch = p.restart && !tileChanged && !p.filt && !p.clearBehind;
	p.maxPL = primeRef ? LH2_MAX_BOUNCES : maxPathLength;
	/* no specular event and no alpha cut-out in any material: every path ends at its second vertex,
	   so the bounce after it would be empty; not launching it saves three launches (~25 us) */
	if (!primeRef && diffuseOnly) p.maxPL = std::min( p.maxPL, 2 );
	/* the path tail (setting "pathTail"): bounces pathTail .. maxPL in one launch of k_trace_path4d */
	p.tailL = (!primeRef && !p.filt && pathTail >= 2 && pathTail <= p.maxPL && TraceVersion() == 7) ? pathTail : 0;
	/* early shade: the first shade launch follows the primary launch on the ahead stream and writes the ping-pong buffer
	   the previous frame's launches after its overlap event do not use (PathStreams::busy / earlyOk).  Only when this
	   frame has a path tail from bounce 3 on: else its first shade launch is its overlap event (and, with the tail from
	   bounce 2, its shadow snapshot), and on the ahead stream neither would follow the previous frame's finalize (the
	   side shadow launch and the next frames' early shades would add into the accumulator and the delta before the
	   previous frame is finalized) */
	p.early = p.pFrame && !p.serialize && earlyShade && frameOverlap == 1 && ps.earlyOk && p.small && p.tailL >= 3;
	/* without lights no path samples one (RandomPointOnLight: lightPdf 0), so there are no shadow
	   rays and their launches are not queued */
	p.shadows = nArea + nPoint + nSpot + nDir > 0;
	/* shadow overlap: the shade launch before the tail snapshots the queued shadow rays (advance_bounce), and the side
	   launch traces them beside the tail */
	p.overlap = p.shadows && p.tailL && shadowOverlap;
	/* RenderCore_PrimeRef traces the shadow rays of every bounce right after it, and hands off to the next bounce in a
	   launch of its own after that (their counts are reset first); else one shadow launch ends the frame */
	p.bounceShadows = primeRef && p.shadows, p.finalShadows = !primeRef && p.shadows, p.handOffLaunch = primeRef;
	p.terminal = !primeRef && !p.filt && !p.shadows && !canEmit && terminalShade;
	p.hvFactor = packetHeavy > 0 ? packetHeavy : p.tailL ? 3.0f : 2.0f;
	/* the next frame's primary launch starts after this frame's first shade launch (the last reader of the primary
	   buffers), or (frameOverlap 1) after the shade launch before the path tail: beside the latency-bound tail */
	p.overlapL = frameOverlap == 1 && p.tailL ? p.tailL - 1 : 1;
	/* a bounce launch the next frame's primary launch will likely run beside (this frame overlapped: the next one
	   probably does too): fewer blocks per CU, so the packets' latency-bound waves get slots from the start instead
	   of the bounce launch's tail (config 2: 4262-4296 -> 4437-4442 Mrays/s at 5, r03q_ab_trace_blocks.txt), and the
	   7-wave variant (8 waves slow the packets beside the launch, r04ad) */
	p.besideNext = !p.serialize && p.fusedCam;
	p.besideGrid = smCount * std::min( blocksPerCU, kOverlapTraceBlocks );
	/* traceWaves 0: the 7-wave variant for every scene (round 6: instanced scenes too, with the early node loads), on its occupancy's grid */
	p.traceWaves = ScenePicksWaves();
	p.closestGrid = smCount * ClosestBlocksPerCU( p.traceWaves );
	p.primaryGrid = p.packets ? PacketGrid() : p.closestGrid;
	/* the path tail's kernel variant (pathTailWaves 0): 4 waves per SIMD (128 VGPRs) for every frame since the shade batches write their
	   shadow rays at once (its spills 68 -> 40 VGPRs; small frames: config 3 -0.8 %, profiles/r06s_ab_tail_waves.txt); 3
	   (no spills) was the small frames' variant before */
	p.tailWaves = pathTailWaves == 3 || pathTailWaves == 4 ? (uint32_t)pathTailWaves : 4u;
	/* with the overlap the path tail runs fewer blocks per CU and leaves registers for the side launch's waves
	   (pathTailBlocks; 0: 3 for small frames, whose tail phase is the frame's longest, else 2) */
	const int occ = p.tailWaves == 4 ? pathBlocksPerCU4 : pathBlocksPerCU;
	const int ptBlocks = pathTailBlocks > 0 ? pathTailBlocks : p.overlap ? (p.small ? 3 : 2) : occ;
	p.tailGrid = smCount * std::min( std::min( blocksPerCU, occ ), ptBlocks );
	/* the global stacks (sideStack, gstack) are sized for maxBlocksPerCU blocks per CU: the shadow grids stay within it */
	const int sb = sideBlocks >= 0 ? sideBlocks : p.small ? 3 : 4;
	p.sideGrid = sb > 0 ? smCount * std::min( sb, maxBlocksPerCU ) : p.traceGrid;
	p.finalShadowGrid = finalShadowBlocks > 0 ? smCount * std::min( finalShadowBlocks, maxBlocksPerCU ) : p.traceGrid;
	return p;
}

/* the frame's state transitions and buffers; `f` gets the scene and the frame parity's slots */
void RenderCore::BeginFrame( Frame& f, int converge )
{
	const FramePlan& p = f.plan;
	if (p.restart)
	{
		samplesTaken = 0;
		firstConvergingFrame = true;
		camRNGseed = 0x12345678;
	}
	if (converge == LH2_CONVERGE) firstConvergingFrame = false;
	/* converge == Restart resets the history (the first converging frame after it restarts the accumulation too, as in the
	   reference, but keeps the history) */
	if (p.filt && converge == LH2_RESTART) fl.historyValid = false;
	f.sd = MakeSceneDev();
	f.tlas = accel.Slot();
	if (p.clearAll) CHK_HIP( hipMemsetAsync( accumulator.ptr, 0, sizeof( float4 ) * (size_t)scrwidth * scrheight, stream ) );
	EnsurePaths( p.pathCount );
	/* shadow rays in segments of shadowStride */
	ps.count = p.pathCount, ps.segStride = p.segStride, ps.shadowStride = (uint32_t)(ps.shCap / LH2_SEGS);
	ps.fp ^= 1;
	f.s = Slots();
	if (p.filt) CHK_HIP( hipMemsetAsync( accumulator.ptr, 0, sizeof( float4 ) * 2 * (size_t)scrwidth * scrheight, stream ) );
	if (p.hvRelayout)
	{
		ps.hvCap = p.hvCap, ps.hvMaskWords = (LH2_SEGS * p.hvCap + 31) / 32;
		ps.hvBlock = LH2_HV_MASK + ps.hvMaskWords + LH2_SEGS * p.hvCap, ps.hvParity = 0;
		ps.hv.resize( 2 * (size_t)ps.hvBlock );
		CHK_HIP( hipMemsetAsync( ps.hv.ptr, 0, sizeof( uint32_t ) * 2 * ps.hvBlock, stream ) );
		ps.relaid = true;
	}
	if (p.clearBehind) CHK_HIP( hipMemsetAsync( accumulator.ptr, 0, sizeof( float4 ) * (size_t)scrwidth * scrheight, stream ) );
}

/* the closest-hit launch of bounce `pathLength` over the rays of `rays`: the bounce's paths (the path counts ping-pong,
   Counters::segPath) and its work-queue heads (the primary launch's: kPrimarySlot) */
TraceArgs RenderCore::BounceArgs( const Frame& f, int pathLength, const PathSet& rays ) const
{
	TraceArgs ta{};
	ta.version = TraceVersion();
	rays.Rays( ta );
	ta.segCounts = f.s.c->segPath[(pathLength - 1) & 1], ta.segStride = f.plan.segStride, ta.segBack = f.s.c->segBack[(pathLength - 1) & 1];
	ta.cursor = f.s.Cursor( pathLength );
	ta.refill = (uint32_t)refillOther, ta.leafBatch = (uint32_t)leafBatch;
	ta.gstack = ps.gstack.ptr;
	return ta;
}

/* what the shade launch of a bounce and the path tail share */
ShadeParams RenderCore::ShadeArgs( const Frame& f, int pathLength ) const
{
	ShadeParams sp{};
	sp.shadowStride = ps.shadowStride;
	sp.shO = f.s.shO, sp.shD = f.s.shD, sp.shP = f.s.shP;
	sp.acc = accumulator.ptr, sp.counters = f.s.c;
	sp.w = scrwidth, sp.h = scrheight, sp.pass = samplesTaken, sp.pathLength = pathLength, sp.maxPathLength = f.plan.maxPL;
	sp.probePixel = probeX + scrwidth * probeY;
	sp.spreadAngle = f.view.spreadAngle;
	if (f.plan.filt)
	{
		sp.fFeatures = fl.features.ptr, sp.fWorldPos = fl.worldPos[fl.cur].ptr, sp.fDeltaDepth = fl.deltaDepth.ptr;
		sp.fPos = f.cp.pos, sp.fP1 = f.cp.p1, sp.fRight = f.cp.right, sp.fUp = f.cp.up;
	}
	return sp;
}

/* the hand-off from bounce `pathLength` to the next one; before the path tail it also takes the shadow overlap's snapshot */
BounceAdvance RenderCore::HandOff( const Frame& f, int pathLength ) const
{
	Counters* const c = f.s.c;
	const int cur = (pathLength - 1) & 1, next = pathLength & 1;
	const bool beforeTail = pathLength + 1 == f.plan.tailL, snap = f.plan.overlap && beforeTail;
	return { c->segPath[next], c->segBack[next], c->segPath[cur], c->segBack[cur], f.s.rayLog, ps.activeLog, beforeTail,
		snap ? f.s.shSnap : nullptr, snap ? f.s.Cursor( LH2_SHADOW_SLOT ) : nullptr };
}

/* a shadow launch with fused finalizeConnections (rendercore.cpp:575-592) over this frame's shadow stream */
TraceArgs RenderCore::ShadowArgs( const FrameSlots& s, const uint32_t* segCounts, int cursorSlot, int leafBatch, int* gstack ) const
{
	TraceArgs ta{};
	ta.version = TraceVersion();
	ta.rayO = s.shO, ta.rayD = s.shD, ta.segCounts = segCounts, ta.segStride = ps.shadowStride;
	ta.cursor = s.Cursor( cursorSlot );
	ta.refill = (uint32_t)refillOther, ta.leafBatch = (uint32_t)leafBatch;
	ta.mask = s.shMask, ta.potentials = s.shP, ta.acc = accumulator.ptr, ta.gstack = gstack;
	return ta;
}

void RenderCore::LaunchClosest( const Frame& f, const TraceArgs& ta, int grid, int pathLength, hipStream_t st )
{
#ifdef LH2_TOUCH
	TouchBegin();
#endif
	lh2_launch_trace_closest( &f.sd, &ta, grid, { nullptr, ps.evTrace[pathLength] }, st );
#ifdef LH2_TOUCH
	TouchReport( pathLength );
#endif
}

/* primary rays (camera.h) for every sample of the tile, and their trace launch: the camera fused into the primary packet
   launch, or a camera launch and a closest-hit launch (packets or per ray) */
void RenderCore::PrimaryStage( Frame& f )
{
	const FramePlan& p = f.plan;
	CameraParams& cp = f.cp;
	SetCameraView( cp, f.view );
	cp.aperture = p.aperture, cp.distortion = f.view.distortion, cp.geometryEpsilon = geometryEpsilon;
	cp.w = scrwidth, cp.h = scrheight, cp.pass = samplesTaken;
	cp.R0 = XorShift( camRNGseed );
	cp.y0 = std::max( 0, tileY0 ), cp.tileRows = p.tileRows;
	cp.band = tileBand > 0 ? tileBand : std::max( 1, p.tileRows ), cp.bandStride = tileBand > 0 ? tileStride : std::max( 1, p.tileRows );
	cp.tiled = tiledRays;
	cp.primeRef = primeRef;
	/* the camera launch (or the fused primary launch) also resets the frame's counters and work-queue heads */
	cp.initC = f.s.c, cp.cursors = f.s.cursors, cp.cursorWords = LH2_CURSOR_SLOTS * LH2_CURSOR_WORDS;
	cp.pathCount = p.pathCount, cp.segStride = p.segStride;
	cp.clearAcc = p.clearByLaunch ? accumulator.ptr : nullptr;
	/* heavy-first primary packets: the block the previous frame recorded, and the other one, which the camera launch zeroes */
	uint32_t *hvRead = nullptr, *hvWrite = nullptr;
	if (p.hvOn)
	{
		hvRead = ps.hv.ptr + (size_t)ps.hvParity * ps.hvBlock, hvWrite = ps.hv.ptr + (size_t)(1 - ps.hvParity) * ps.hvBlock;
		cp.hvZero = hvWrite, cp.hvZeroWords = LH2_HV_MASK + ps.hvMaskWords;
		ps.hvParity = 1 - ps.hvParity;
	}
	hipStream_t primStream = stream;
	cp.keepCursor = -1;   /* a camera launch behind the previous frame resets every work-queue head */
	if (p.pFrame)
	{
		/* beside the previous frame (on the ahead stream, after the previous frame's shade launch before its path tail, or
		   its first without one: the last reader of the primary buffers and of the heavy-packet block this frame records
		   into) or behind it (core stream), the primary stage does the frame's resets itself (this frame parity's counters
		   and heads, whose last user, the frame before the previous one, is done: no launch, and its gap, before it;
		   profiles/r05f_ab_primary_resets.txt).  Its own work-queue heads (kPrimarySlot) are left alone */
		primStream = p.serialize ? stream : aheadStream;
		cp.keepCursor = kPrimarySlot * LH2_CURSOR_WORDS;
		if (!p.serialize) CHK_HIP( hipStreamWaitEvent( aheadStream, ps.overlapEv, 0 ) );
		if (p.hvOn && !ps.hvNextZeroed) CHK_HIP( hipMemsetAsync( cp.hvZero, 0, sizeof( uint32_t ) * cp.hvZeroWords, primStream ) );
		cp.hvZero = nullptr, cp.hvZeroWords = 0;
		ps.relaid = false;
	}
	ps.hvNextZeroed = false;
	f.in = p.early ? ps.busy : 0;
	ps.earlyOk = false;
	/* the frame's start: a marker before the camera launch (~4 us of idle GPU), not the launch's own start
	   event (hipExtLaunchKernelGGL start events cost ~8 us: tools/launch_gap.hip, profiles/r02q_launch_gap.txt) */
	CHK_HIP( hipEventRecord( evFrame[0], primStream ) );
	/* a frame whose primary stage may run beside the previous frame keeps its primary rays apart from the bounce ping-pong */
	const PathSet prim = p.pFrame ? ps.Primary( ps.fp ) : ps.Bounce( f.in );
	if (p.fusedCam) ps.prevStop = evFrame[0];
	else
	{
		lh2_launch_camera( &cp, dBlueNoise.ptr, prim.O, prim.D, prim.T4, prim.Q4, (int)p.pathCount, { nullptr, ps.evCamera }, primStream );
		ps.prevStop = ps.evCamera;
	}
	if (p.restart) tileChanged = false;
	TraceArgs ta = BounceArgs( f, 1, prim );
	ta.packet = p.packets;
	if (p.hvOn)
	{
		ta.hvRead = f.hvReadBlock = hvRead, ta.hvWrite = hvWrite;
		ta.hvCap = ps.hvCap, ta.hvMaskWords = ps.hvMaskWords, ta.hvFactor = p.hvFactor, ta.hvTiles = p.hvTiles;
	}
	if (p.fusedCam)
	{
		/* the paths are dense (camera order): fixed counts, no segment counters */
		ta.segCounts = nullptr, ta.segBack = nullptr, ta.countFixed = p.pathCount;
		lh2_launch_trace_primary( &f.sd, &ta, &cp, prim.T4, prim.Q4, PacketGrid(), { nullptr, ps.evTrace[1] }, primStream );
	}
	else
	{
		/* after its camera launch (the camera's resets set the dense segment counts); beside the previous frame it walks
		   with a global stack of its own */
		ta.traceWaves = (uint32_t)p.traceWaves;
		if (primStream != stream) ta.gstack = ps.aheadStack.ptr;
		LaunchClosest( f, ta, p.primaryGrid, 1, primStream );
	}
	/* the core stream waits for a primary launch beside the previous frame, unless the first shade launch follows it there */
	if (primStream != stream && !p.early) CHK_HIP( hipStreamWaitEvent( stream, ps.evTrace[1], 0 ) );
	ps.Stamp( ps.fromTrace[1], ps.evTrace[1] );
}

/* bounces 2 .. of the path: a closest-hit launch; beside the next frame's primary launch (FramePlan::besideNext) a smaller one */
void RenderCore::TraceBounce( Frame& f, int pathLength )
{
	const FramePlan& p = f.plan;
	const bool beside = p.besideNext && pathLength > p.overlapL;
	TraceArgs ta = BounceArgs( f, pathLength, ps.Bounce( f.in ) );
	ta.traceWaves = beside ? 7u : (uint32_t)p.traceWaves;
	LaunchClosest( f, ta, beside ? p.besideGrid : p.closestGrid, pathLength, stream );
	ps.Stamp( ps.fromTrace[pathLength], ps.evTrace[pathLength] );
}

/* the shade launch of a bounce: its last block hands off to the next bounce (no launch of its own; FramePlan::handOffLaunch:
   a launch does).  The first bounce of a frame with a primary stage of its own reads the primary buffers */
void RenderCore::ShadeBounce( Frame& f, int pathLength )
{
	const FramePlan& p = f.plan;
	Counters* const c = f.s.c;
	ShadeParams sp = ShadeArgs( f, pathLength );
	sp.segCounts = c->segPath[(pathLength - 1) & 1], sp.segOut = c->segPath[pathLength & 1], sp.segStride = p.segStride;
	sp.segBack = c->segBack[(pathLength - 1) & 1], sp.segOutBack = c->segBack[pathLength & 1];
	/* two-ended path segments: rays with a chord through the scene box below chordSplit x its largest
	   extent go last (setting "chordSplit"; 0: off) */
	const float *sceneLo = accel.WorldLo(), *sceneHi = accel.WorldHi();
	const float ext = std::max( std::max( sceneHi[0] - sceneLo[0], sceneHi[1] - sceneLo[1] ), sceneHi[2] - sceneLo[2] );
	for (int k = 0; k < 3; k++) sp.chordLo[k] = sceneLo[k], sp.chordHi[k] = sceneHi[k];
	sp.chordCut = ext > 0 ? chordSplit * ext : 0.0f;
	sp.advance = pathLength < p.maxPL && !p.handOffLaunch;
	sp.adv = HandOff( f, pathLength );
	f.snapped = f.snapped || sp.adv.shadowSnap;
	(pathLength == 1 && p.pFrame ? ps.Primary( ps.fp ) : ps.Bounce( f.in )).In( sp );
	ps.Bounce( 1 - f.in ).Out( sp );
	sp.primeRef = primeRef;
	sp.terminal = p.terminal && pathLength > 1;
	sp.R0 = (uint32_t)samplesTaken * 7907u + (uint32_t)pathLength * 91771u;
	if (pathLength == 1 && p.fusedCam && f.hvReadBlock)
	{
		/* the block this frame's packets read is the one the next frame records into */
		sp.hvZero = f.hvReadBlock, sp.hvZeroWords = LH2_HV_MASK + ps.hvMaskWords;
		ps.hvNextZeroed = true;
	}
	const bool earlyHere = p.early && pathLength == 1;
	if (earlyHere) sp.acc = f.s.delta;   /* the previous frame's finalize may not have read the accumulator yet */
	lh2_launch_shade( &f.sd, &sp, p.shadeGrid, { nullptr, ps.evShade[pathLength] }, earlyHere ? aheadStream : stream );
	if (earlyHere) CHK_HIP( hipStreamWaitEvent( stream, ps.evShade[pathLength], 0 ) );
	ps.Stamp( ps.fromShade[pathLength], ps.evShade[pathLength] );
	if (pathLength == 1 || pathLength == p.overlapL)
	{
		/* the next frame's primary launch starts after this launch (FramePlan::overlapL: the final one).  After it only the
		   path tail (in place) or the last bounce (no extension rays) runs: both use the buffer this launch writes, 1 - f.in */
		ps.overlapEv = ps.evShade[pathLength];
		ps.busy = 1 - f.in;
		ps.earlyOk = p.tailL && pathLength == p.tailL - 1;   /* config 2 (no tail): no gain, and the fold costs (r04b) */
	}
}

/* the path tail: trace and shade every remaining bounce in one launch; each path's records are updated in place, its
   shadow rays queued for the shadow launch, and rayLog counted.  No shade interval of its own (Synchronize) */
void RenderCore::PathTail( Frame& f, int pathLength )
{
	const FramePlan& p = f.plan;
	const PathSet io = ps.Bounce( f.in );
	TraceArgs ta = BounceArgs( f, pathLength, io );
	ta.shadeBatch = (uint32_t)pathTailBatch, ta.tailWaves = p.tailWaves;
	ShadeParams sp = ShadeArgs( f, pathLength );
	io.In( sp ), io.Out( sp );
	sp.hits = nullptr;   /* the tail shades the hits it finds itself */
	sp.adv.rayCountLog = f.s.rayLog;
	lh2_launch_trace_path( &f.sd, &ta, &sp, p.tailGrid, { nullptr, ps.evTrace[pathLength] }, stream );
	if (p.overlap)
	{
		/* the shadow rays of the bounces before the tail, beside it on the side stream (segment counts:
		   the snapshot; the final launch's work-queue heads start behind them) */
		CHK_HIP( hipStreamWaitEvent( sideStream, ps.prevStop, 0 ) );
		const TraceArgs ts = ShadowArgs( f.s, f.s.shSnap, LH2_SHADOW_SLOT + 1, kShadowLeafBatch, ps.sideStack.ptr );
		lh2_launch_trace_any( &f.sd, &ts, p.sideGrid, 1, { nullptr, ps.evSide }, sideStream );
		ps.fromSide = ps.prevStop;
		f.sideOn = true;
	}
	ps.Stamp( ps.fromTrace[pathLength], ps.evTrace[pathLength] );
	f.tailL = pathLength;
}

/* the bounce loop: the primary rays are traced already (PrimaryStage); bounce 1 only shades them */
void RenderCore::BounceLoop( Frame& f )
{
	const FramePlan& p = f.plan;
	for (int pathLength = 1; pathLength <= p.maxPL; pathLength++)
	{
		f.pl = pathLength;
		if (pathLength == p.tailL) { PathTail( f, pathLength ); break; }
		if (pathLength > 1) TraceBounce( f, pathLength );
		ShadeBounce( f, pathLength );
		if (pathLength == p.maxPL) break;
		if (p.bounceShadows)
		{
			const TraceArgs ts = ShadowArgs( f.s, f.s.c->segShadow, LH2_MAX_BOUNCES + pathLength, leafBatch, ps.gstack.ptr );
			lh2_launch_trace_any( &f.sd, &ts, p.traceGrid, 1, { nullptr, ps.evShadowB[pathLength] }, stream );
			ps.Stamp( ps.fromShadowB[pathLength], ps.evShadowB[pathLength] );
		}
		/* the hand-off writes this bounce's extension-ray count into the pinned activeLog itself */
		ps.countReady[pathLength] = ps.evShade[pathLength];
		if (p.handOffLaunch)
		{
			const BounceAdvance adv = HandOff( f, pathLength );
			lh2_launch_counters_next( f.s.c, &adv, pathLength, 1, { nullptr, ps.evCount[pathLength] }, stream );
			ps.prevStop = ps.countReady[pathLength] = ps.evCount[pathLength];
		}
		/* early exit without stalling the GPU: wait for the count of the previous bounce while this one is
		   queued; when it was 0, this bounce is empty and so is everything after it */
		if (pathLength >= 2)
		{
			CHK_HIP( hipEventSynchronize( ps.countReady[pathLength - 1] ) );
			if (ps.activeLog[pathLength - 1] == 0) break;
		}
		f.in = 1 - f.in;
	}
	/* an early frame whose paths all ended before the shade launch before its path tail (pathTail >= 4, e.g. every primary
	   ray misses): its overlap event is still its first shade launch, on the ahead stream, which never waited for the
	   previous frame's finalize; the next frame's counter resets on this parity's block two frames on order themselves after
	   overlapEv only.  So it moves to the core stream, behind the previous frame's finalize */
	if (p.early && ps.overlapEv == ps.evShade[1])
	{
		CHK_HIP( hipEventRecord( ps.evEarlyEnd, stream ) );
		ps.overlapEv = ps.evEarlyEnd;
	}
}

/* the frame's shadow rays (those the side launch did not take) + fused finalizeConnections (rendercore.cpp:575-592) */
void RenderCore::FinalShadows( Frame& f )
{
	/* a snapshot whose side launch did not happen (the frame ended before its path tail): the final launch
	   traces every shadow ray, from the first */
	if (f.snapped && !f.sideOn)
		CHK_HIP( hipMemsetAsync( f.s.Cursor( LH2_SHADOW_SLOT ), 0, sizeof( uint32_t ) * LH2_CURSOR_WORDS, stream ) );
	if (!f.plan.finalShadows) return;
	const TraceArgs ta = ShadowArgs( f.s, f.s.c->segShadow, LH2_SHADOW_SLOT, kShadowLeafBatch, ps.gstack.ptr );
	lh2_launch_trace_any( &f.sd, &ta, f.plan.finalShadowGrid, 1, { nullptr, ps.evShadow }, stream );
	ps.fromShadow = ps.prevStop;
}

/* the side-stream join, the filter chain or the finalize launch, the display copy and the record of the frame */
void RenderCore::FinishFrame( Frame& f )
{
	const FramePlan& p = f.plan;
	/* the side launch's contributions are in the accumulator before the frame is finalized */
	if (f.sideOn) CHK_HIP( hipStreamWaitEvent( stream, ps.evSide, 0 ) );
	samplesTaken += scrspp;
	/* finalize also delivers the frame's counters and ray-count log, and the scene error, to hostStats */
	const FrameStatsDev fs{ f.s.c, f.s.rayLog + 1, &hostStats->counters, hostStats->rayCount + 1, accel.SceneErr( f.tlas ), &hostStats->sceneError,
		f.s.Cursor( kPrimarySlot ), p.early ? f.s.delta : nullptr };
	/* a tile finalizes its own rows only (a rank of the band partition: the gathered frame is finalized
	   where it is assembled, MultiDevice / FinalizeFrame) */
	RowMap rm{};
	if (p.tileRows < scrheight) rm = { scrwidth, f.cp.y0, f.cp.band, f.cp.bandStride, p.tileRows };
	/* the previous frame's end stays recorded (evFrame[2]): an overlapped frame's render time starts at the later of
	   its primary launch's start and the previous frame's end (Synchronize), so per-frame times sum to wall time */
	std::swap( evFrame[1], evFrame[2] );
	prevFrameEndValid = frameEndRecorded;
	if (p.filt)
	{
		/* the filter chain writes the frame; the finalize launch only delivers the statistics (no pixels).  The next frame stays
		   behind this one */
		RunFilter( f.view, p.taa );
		lh2_launch_finalize( accumulator.ptr, frame.ptr, 0, 1.0f, &fs, { nullptr, evFrame[1] }, stream, nullptr );
		ps.relaid = true;
	}
	else lh2_launch_finalize( accumulator.ptr, frame.ptr, scrwidth * scrheight, 1.0f / (float)samplesTaken, &fs, { nullptr, evFrame[1] }, stream, &rm );
	frameEndRecorded = true;
	accel.ReleaseSlot( f.tlas, stream );   /* the next update of this TLAS slot waits for it */
	if (glResource && !displayAtFinalize) CopyFrameToDisplay();
	hostStats->rayCount[0] = ps.count;
	ps.lastFused = p.pFrame, ps.lastSceneVersion = sceneVersion;
	last = { f.pl, f.tailL, f.tailL ? p.maxPL : f.pl, p.early, f.sideOn, p.shadows, primeRef != 0, p.filt, p.pFrame && !p.serialize, p.taa };
	statsPending = true;
}

/* the finalized frame into the registered GL texture (SetInteropTexture) */
void RenderCore::CopyFrameToDisplay()
{
	hipArray_t arr = nullptr;
	CHK_HIP( hipGraphicsMapResources( 1, &glResource, stream ) );
	CHK_HIP( hipGraphicsSubResourceGetMappedArray( &arr, glResource, 0, 0 ) );
	CHK_HIP( hipMemcpy2DToArrayAsync( arr, 0, 0, frame.ptr, sizeof( float4 ) * scrwidth, sizeof( float4 ) * scrwidth, scrheight, hipMemcpyDeviceToDevice, stream ) );
	CHK_HIP( hipGraphicsUnmapResources( 1, &glResource, stream ) );
}


/* the denoise chain of a frame (reference rendercore.cpp:827-862): prepare, three a-trous passes (the last one writes the
   frame), then the buffers change roles for the next frame.  With taa (setting "TAA") the last pass writes fl.linear, the
   TAA pass blends it into this frame's TAA pixels and the unsharpen writes the frame from those */
void RenderCore::RunFilter( const lh2_ViewPyramid& view, bool taa )
{
	const int c = fl.cur, q = 1 - c;
	CHK_HIP( hipEventRecord( fl.ev[0], stream ) );
	FilterPrepareArgs pa{};
	pa.acc = accumulator.ptr, pa.features = fl.features.ptr;
	pa.worldPos = fl.worldPos[c].ptr, pa.prevWorldPos = fl.worldPos[q].ptr, pa.deltaDepth = fl.deltaDepth.ptr;
	pa.prevMoments = fl.moments[q].ptr;
	pa.shading = fl.shading.ptr, pa.motion = fl.motion.ptr, pa.moments = fl.moments[c].ptr;
	lh2_filter_view( fl.historyValid ? &fl.prevView : &view, scrheight, pa.prevView );
	lh2_filter_view( &view, scrheight, pa.curView );
	pa.w = scrwidth, pa.h = scrheight, pa.scale = 1.0f / (float)scrspp;
	pa.clampDirect = clampDirect, pa.clampIndirect = clampIndirect;
	pa.camStationary = !fl.historyValid || !memcmp( &fl.prevView, &view, sizeof( lh2_float3 ) * 4 );
	pa.historyValid = fl.historyValid;
	lh2_launch_filter_prepare( &pa, { nullptr, fl.ev[1] }, stream );
	FilterAtrousArgs aa{};
	aa.features = fl.features.ptr, aa.worldPos = fl.worldPos[c].ptr, aa.prevWorldPos = fl.worldPos[q].ptr, aa.deltaDepth = fl.deltaDepth.ptr;
	aa.motion = fl.motion.ptr, aa.moments = fl.moments[c].ptr;
	aa.w = scrwidth, aa.h = scrheight, aa.historyValid = fl.historyValid;
	/* filtered[q] holds the previous frame's first pass: this frame's goes to filtered[c], the second pass then overwrites
	   filtered[q], and the third writes the frame */
	float4* const in[3] = { fl.shading.ptr, fl.filtered[c].ptr, fl.filtered[q].ptr };
	float4* const out[3] = { fl.filtered[c].ptr, fl.filtered[q].ptr, taa ? fl.linear.ptr : frame.ptr };
	for (int phase = 1; phase <= 3; phase++)
	{
		aa.phase = phase, aa.A = in[phase - 1], aa.B = phase == 1 ? fl.filtered[q].ptr : nullptr, aa.C = out[phase - 1];
		aa.lds = filterLds >= 0 ? filterLds : kFilterLdsPick[phase - 1];
		lh2_launch_filter_atrous( &aa, { nullptr, fl.ev[phase + 1] }, stream );
	}
	if (taa)
	{
		FilterTaaArgs ta{};
		ta.in = fl.linear.ptr, ta.prev = fl.taa[q].ptr, ta.motion = fl.motion.ptr, ta.out = fl.taa[c].ptr;
		ta.w = scrwidth, ta.h = scrheight, ta.historyValid = fl.historyValid && fl.taaValid;
		ta.lds = filterLds >= 0 ? filterLds : kTaaLdsPick;
		lh2_launch_filter_taa( &ta, { nullptr, fl.ev[5] }, stream );
		ta.in = fl.taa[c].ptr, ta.prev = nullptr, ta.motion = nullptr, ta.out = frame.ptr;
		lh2_launch_filter_unsharpen( &ta, { nullptr, fl.ev[6] }, stream );
		fl.taaValid = true;
	}
	/* the next frame: worldPos, moments and the first pass's output become its history (the swaps of rendercore.cpp:856-862) */
	fl.cur = q, fl.historyValid = true, fl.prevView = view;
}

void RenderCore::GetFilterBuffer( int which, void* out )
{
	Synchronize();
	if (!fl.pixels) FatalError( "the denoise mode is off (setting \"filter\"): it has no buffers" );
	const size_t n = fl.pixels;
	const int c = 1 - fl.cur, q = fl.cur;   /* the last frame's buffers, and the ones of the frame before it */
	const void* src = nullptr;
	size_t bytes = 16 * n;
	switch (which)
	{
	case LH2_FILTER_BUF_ACC: src = accumulator.ptr, bytes = 32 * n; break;
	case LH2_FILTER_BUF_FEATURES: src = fl.features.ptr; break;
	case LH2_FILTER_BUF_WORLDPOS: src = fl.worldPos[c].ptr; break;
	case LH2_FILTER_BUF_DELTADEPTH: src = fl.deltaDepth.ptr; break;
	case LH2_FILTER_BUF_MOTION: src = fl.motion.ptr, bytes = 8 * n; break;
	case LH2_FILTER_BUF_MOMENTS: src = fl.moments[c].ptr; break;
	case LH2_FILTER_BUF_SHADING: src = fl.shading.ptr; break;
	case LH2_FILTER_BUF_PHASE1: src = fl.filtered[c].ptr; break;
	case LH2_FILTER_BUF_PHASE2: src = fl.filtered[q].ptr; break;
	case LH2_FILTER_BUF_PHASE3: src = last.taa ? fl.linear.ptr : frame.ptr; break;
	case LH2_FILTER_BUF_PREVWORLDPOS: src = fl.worldPos[q].ptr; break;
	case LH2_FILTER_BUF_PREVMOMENTS: src = fl.moments[q].ptr; break;
	case LH2_FILTER_BUF_TAA: case LH2_FILTER_BUF_PREVTAA:
		if (!fl.taaPixels) FatalError( "the TAA stage is off (settings \"filter\" and \"TAA\"): it has no buffers" );
		src = fl.taa[which == LH2_FILTER_BUF_TAA ? c : q].ptr;
		break;
	default: FatalError( "unknown filter buffer %d", which );
	}
	CHK_HIP( hipMemcpy( out, src, bytes, hipMemcpyDeviceToHost ) );
}
void RenderCore::GetFilterTimes( float* ms4 )
{
	Synchronize();
	for (int k = 0; k < 4; k++) ms4[k] = last.filtered ? fl.ms[k] : 0.0f;
}
void RenderCore::GetTaaTimes( float* ms2 )
{
	Synchronize();
	for (int k = 0; k < 2; k++) ms2[k] = last.filtered && last.taa ? fl.ms[4 + k] : 0.0f;
}

/* k_filter_taa (stage 0) or k_filter_unsharpen (stage 1) on host arrays (lh2_TaaUnit): upload, one launch, copy back.  The
   core's own frame state is not touched */
void RenderCore::TaaUnit( const lh2_TaaUnit& u )
{
	if (u.w < 1 || u.h < 1 || (uint64_t)u.w * u.h > (1u << 26) || u.stage < 0 || u.stage > 1) FatalError( "bad taa unit: stage %d, %d x %d", u.stage, u.w, u.h );
	const size_t n = (size_t)u.w * u.h;
	if (!u.in || !u.out || (u.stage == 0 && (!u.prev || !u.motion))) FatalError( "taa unit: null array" );
	DevBuf<float4> in, prev, out; DevBuf<float2> motion;
	in.upload( (const float4*)u.in, n, stream ), out.resize( n );
	FilterTaaArgs ta{};
	ta.in = in.ptr, ta.out = out.ptr, ta.w = u.w, ta.h = u.h, ta.historyValid = u.historyValid, ta.lds = u.lds;
	if (u.stage == 0)
	{
		prev.upload( (const float4*)u.prev, n, stream ), motion.upload( (const float2*)u.motion, n, stream );
		ta.prev = prev.ptr, ta.motion = motion.ptr;
		lh2_launch_filter_taa( &ta, {}, stream );
	}
	else lh2_launch_filter_unsharpen( &ta, {}, stream );
	CHK_HIP( hipMemcpyAsync( u.out, out.ptr, sizeof( float4 ) * n, hipMemcpyDeviceToHost, stream ) );
	CHK_HIP( hipStreamSynchronize( stream ) );
}

/* one kernel of the chain on host arrays (lh2_FilterUnit): uploads what the stage reads, runs it, copies back what it writes */
void RenderCore::FilterUnit( const lh2_FilterUnit& u )
{
	if (u.w < 1 || u.h < 1 || (uint64_t)u.w * u.h > (1u << 26) || u.stage < 0 || u.stage > 3) FatalError( "bad filter unit: stage %d, %d x %d", u.stage, u.w, u.h );
	const size_t n = (size_t)u.w * u.h;
	auto need = []( const void* p, const char* what ) { if (!p) FatalError( "filter unit: %s is null", what ); };
	need( u.features, "features" ), need( u.worldPos, "worldPos" ), need( u.prevWorldPos, "prevWorldPos" ), need( u.deltaDepth, "deltaDepth" );
	need( u.motion, "motion" ), need( u.moments, "moments" ), need( u.out, "out" );
	DevBuf<uint4> features; DevBuf<float4> worldPos, prevWorldPos, deltaDepth, moments, prevMoments, acc, in, prev, out; DevBuf<float2> motion;
	features.upload( (const uint4*)u.features, n, stream ), worldPos.upload( (const float4*)u.worldPos, n, stream );
	prevWorldPos.upload( (const float4*)u.prevWorldPos, n, stream ), deltaDepth.upload( (const float4*)u.deltaDepth, n, stream );
	out.resize( n ), motion.resize( n ), moments.resize( n );
	if (u.stage == 0)
	{
		need( u.acc, "acc" ), need( u.prevMoments, "prevMoments" );
		acc.upload( (const float4*)u.acc, 2 * n, stream ), prevMoments.upload( (const float4*)u.prevMoments, n, stream );
		FilterPrepareArgs pa{};
		pa.acc = acc.ptr, pa.features = features.ptr, pa.worldPos = worldPos.ptr, pa.prevWorldPos = prevWorldPos.ptr, pa.deltaDepth = deltaDepth.ptr;
		pa.prevMoments = prevMoments.ptr, pa.shading = out.ptr, pa.motion = motion.ptr, pa.moments = moments.ptr;
		lh2_filter_view( &u.prevView, u.h, pa.prevView );
		lh2_filter_view( &u.view, u.h, pa.curView );
		pa.w = u.w, pa.h = u.h, pa.scale = u.scale, pa.clampDirect = u.clampDirect, pa.clampIndirect = u.clampIndirect;
		pa.camStationary = u.camStationary, pa.historyValid = u.historyValid;
		lh2_launch_filter_prepare( &pa, {}, stream );
		CHK_HIP( hipMemcpyAsync( u.features, features.ptr, sizeof( uint4 ) * n, hipMemcpyDeviceToHost, stream ) );
		CHK_HIP( hipMemcpyAsync( u.motion, motion.ptr, sizeof( float2 ) * n, hipMemcpyDeviceToHost, stream ) );
		CHK_HIP( hipMemcpyAsync( u.moments, moments.ptr, sizeof( float4 ) * n, hipMemcpyDeviceToHost, stream ) );
	}
	else
	{
		need( u.in, "in" );
		if (u.stage == 1) need( u.prev, "prev" );
		motion.upload( (const float2*)u.motion, n, stream ), moments.upload( (const float4*)u.moments, n, stream );
		in.upload( (const float4*)u.in, n, stream );
		if (u.stage == 1) prev.upload( (const float4*)u.prev, n, stream );
		FilterAtrousArgs aa{};
		aa.features = features.ptr, aa.worldPos = worldPos.ptr, aa.prevWorldPos = prevWorldPos.ptr, aa.deltaDepth = deltaDepth.ptr;
		aa.motion = motion.ptr, aa.moments = moments.ptr, aa.A = in.ptr, aa.B = u.stage == 1 ? prev.ptr : nullptr, aa.C = out.ptr;
		aa.w = u.w, aa.h = u.h, aa.phase = u.stage, aa.historyValid = u.historyValid, aa.lds = u.lds;
		lh2_launch_filter_atrous( &aa, {}, stream );
	}
	CHK_HIP( hipMemcpyAsync( u.out, out.ptr, sizeof( float4 ) * n, hipMemcpyDeviceToHost, stream ) );
	CHK_HIP( hipStreamSynchronize( stream ) );
}

/* EvaluateBSDF / SampleBSDF on host records (lh2_BsdfUnit) against the uploaded materials: upload, one launch, copy back */
void RenderCore::BsdfUnit( const lh2_BsdfUnit& u )
{
	if (u.n < 0 || u.n > (1 << 24) || (u.sample != 0 && u.sample != 1)) FatalError( "bad bsdf unit: sample %d, n %d", u.sample, u.n );
	if (u.n == 0) return;
	if (!u.in || !u.out) FatalError( "bsdf unit: null array" );
	if (materialCount < 1 || !dMaterials.ptr) FatalError( "bsdf unit: no materials (call SetMaterials first)" );
	for (int i = 0; i < u.n; i++)
	{
		const int mi = (int)lh2_f2b( u.in[(size_t)i * 20 + 3] );
		if (mi < 0 || mi >= materialCount) FatalError( "bsdf unit: sample %d uses material %d of %d", i, mi, materialCount );
	}
	DevBuf<float4> in, out;
	in.upload( (const float4*)u.in, (size_t)u.n * 5, stream );
	out.resize( (size_t)u.n * 2 );
	CHK_HIP( hipMemsetAsync( out.ptr, 0, sizeof( float4 ) * 2 * (size_t)u.n, stream ) );
	lh2_launch_bsdf_unit( dMaterials.ptr, materialCount, in.ptr, out.ptr, u.n, u.sample, stream );
	CHK_HIP( hipGetLastError() );
	CHK_HIP( hipMemcpyAsync( u.out, out.ptr, sizeof( float4 ) * 2 * (size_t)u.n, hipMemcpyDeviceToHost, stream ) );
	CHK_HIP( hipStreamSynchronize( stream ) );
}

void RenderCore::UnpackTile( const void* devSrc, int rank, int nranks, int band )
{
	int rows = 0;
	for (int y = rank * band; y < scrheight; y += nranks * band) rows += std::min( band, scrheight - y );
	lh2_launch_unpack_rows( (const float4*)devSrc, accumulator.ptr, scrwidth, rank * band, band, nranks * band, rows, {}, stream );
}

void RenderCore::FinalizeFrame()
{
	if (!samplesTaken) return;
	lh2_launch_finalize( accumulator.ptr, frame.ptr, scrwidth * scrheight, 1.0f / (float)samplesTaken, nullptr, {}, stream );
	if (glResource) CopyFrameToDisplay();
}

void RenderCore::CopyFrameAsync( void* devDst )
{
	CHK_HIP( hipMemcpyAsync( devDst, frame.ptr, sizeof( float4 ) * (size_t)scrwidth * scrheight, hipMemcpyDeviceToDevice, stream ) );
}

int RenderCore::TileRows() const
{
	if (tileBand > 0)
	{
		int rows = 0;
		for (int y = tileY0; y < scrheight; y += tileStride) rows += std::min( tileBand, scrheight - y );
		return rows;
	}
	const int y0 = std::max( 0, tileY0 ), y1 = tileY1 < 0 ? scrheight : std::min( scrheight, tileY1 );
	return std::max( 0, y1 - y0 );
}

/* shadow rays queued in the segments of the shadow stream (the final shadow pass traces them all) */
static uint32_t QueuedShadowRays( const Counters& c )
{
	uint32_t n = 0;
	for (int k = 0; k < LH2_SEGS; k++) n += c.segShadow[k * LH2_SEGCOUNT_STRIDE];
	return n;
}

void RenderCore::Synchronize()
{
	CHK_HIP( hipStreamSynchronize( aheadStream ) );
	CHK_HIP( hipStreamSynchronize( stream ) );
	if (!statsPending) return;
	statsPending = false;
	const Counters& cn = hostStats->counters;
	bool full = cn.shadowOverflow != 0;
	for (int k = 0; k < LH2_SEGS; k++) full = full || cn.segShadow[k * LH2_SEGCOUNT_STRIDE] > ps.shadowStride;
	if (full) FatalError( "shadow ray buffer overflow" );
	if (hostStats->sceneError) FatalError( "%s: frame skipped", SceneErrorText( hostStats->sceneError ) );
	const uint32_t* rc = hostStats->rayCount;   /* rc[0] = primary; rc[L] = rays traced at pathLength L+1 */
	auto ms = [&]( hipEvent_t a, hipEvent_t b ) { float t = 0; (void)hipEventElapsedTime( &t, a, b ); return t * 1e-3f; };
	/* each interval: the previous launch's stop event -> this launch's stop event (kernel + launch gap) */
	auto trace = [&]( int L ) {
		if (L > last.pl) return 0.0f;
		float t = ms( ps.fromTrace[L], ps.evTrace[L] );
		/* early shade: the second bounce's interval starts at the first shade launch's stop (ahead stream); the part
		   before the previous frame's end is the previous frame's */
		if (L == 2 && last.early && prevFrameEndValid)
		{
			const float shared = ms( ps.fromTrace[L], evFrame[2] );
			if (shared > 0) t = std::max( 0.0f, t - shared );
		}
		return t;
	};
	coreStats.primaryRayCount = rc[0];
	coreStats.traceTime0 = trace( 1 );
	coreStats.bounce1RayCount = last.pathLengths >= 2 ? rc[1] : 0;
	coreStats.traceTime1 = last.pathLengths >= 2 ? trace( 2 ) : 0;
	coreStats.deepRayCount = 0, coreStats.traceTimeX = 0;
	/* (a path tail's bounces past its first have no launch of their own: their time is in its launch) */
	for (int L = 3; L <= last.pathLengths; L++)
	{
		coreStats.deepRayCount = rc[L - 1];
		if (L <= last.pl) coreStats.traceTimeX = trace( L );
	}
	float shadow = 0, shade = 0;
	if (last.shadows && !last.primeRef)
		shadow = ms( ps.fromShadow, ps.evShadow ) + (last.sideOn ? ms( ps.fromSide, ps.evSide ) : 0.0f);
	else if (last.shadows) for (int L = 1; L < last.pl; L++) shadow += ms( ps.fromShadowB[L], ps.evShadowB[L] );
	for (int L = 1; L <= last.pl; L++) if (L != last.tailL) shade += ms( ps.fromShade[L], ps.evShade[L] );
	coreStats.shadowTraceTime = shadow;
	coreStats.shadeTime = shade;
	coreStats.filterTime = 0;
	if (last.filtered)
	{
		const int kernels = last.taa ? 6 : 4;
		coreStats.filterTime = ms( fl.ev[0], fl.ev[kernels] );
		for (int k = 0; k < 6; k++) fl.ms[k] = k < kernels ? ms( fl.ev[k], fl.ev[k + 1] ) * 1e3f : 0.0f;
	}
	for (int L = 1; L <= last.pathLengths && L <= 8; L++) lastKernelMs[L - 1] = trace( L ) * 1e3f;
	coreStats.totalShadowRays = last.primeRef ? cn.totalShadowRays : QueuedShadowRays( cn );
	coreStats.totalExtensionRays = cn.totalExtensionRays;
	coreStats.totalRays = coreStats.totalExtensionRays + coreStats.totalShadowRays;
	/* device time of the whole frame (the reference's Render blocks).  Under frameOverlap the frame's primary launch
	   starts beside the previous frame's tail: the part before the previous frame's end is the previous frame's
	   (ADVICE r3).  traceTime0 stays the primary launch's own duration, stretched by what ran beside it */
	coreStats.renderTime = ms( evFrame[0], evFrame[1] );
	if (last.overlapped && prevFrameEndValid)
	{
		const float shared = ms( evFrame[0], evFrame[2] );
		if (shared > 0) coreStats.renderTime = std::max( 0.0f, coreStats.renderTime - shared );
	}
	coreStats.probedInstid = cn.probedInstid, coreStats.probedTriid = cn.probedTriid, coreStats.probedDist = cn.probedDist;
}

lh2_CoreStats RenderCore::GetCoreStats()
{
	Synchronize();
	coreStats.bvhBuildTime = accel.BuildSeconds();
	return coreStats;
}

void RenderCore::GetRayCounts( uint32_t* out17 )
{
	Synchronize();
	for (int i = 0; i < 16; i++) out17[i] = i < last.pathLengths ? hostStats->rayCount[i] : 0u;
	out17[16] = last.primeRef ? hostStats->counters.totalShadowRays : QueuedShadowRays( hostStats->counters );
}

int RenderCore::DebugShadowRays( float* o4, float* d4, float* p4, int cap )
{
	Synchronize();
	int n = 0;
	const FrameSlots s = Slots();   /* the last frame's parity */
	for (int k = 0; k < LH2_SEGS; k++)
	{
		const uint32_t cnt = std::min( hostStats->counters.segShadow[k * LH2_SEGCOUNT_STRIDE], ps.shadowStride );
		const int m = std::min( (int)cnt, cap - n );
		if (m <= 0) break;
		const size_t at = (size_t)k * ps.shadowStride;
		CHK_HIP( hipMemcpy( o4 + 4 * (size_t)n, s.shO + at, 16 * (size_t)m, hipMemcpyDeviceToHost ) );
		CHK_HIP( hipMemcpy( d4 + 4 * (size_t)n, s.shD + at, 16 * (size_t)m, hipMemcpyDeviceToHost ) );
		CHK_HIP( hipMemcpy( p4 + 4 * (size_t)n, s.shP + at, 16 * (size_t)m, hipMemcpyDeviceToHost ) );
		n += m;
	}
	return n;
}

int RenderCore::DebugBvh4( float* f32Nodes, uint32_t* qNodes, int cap )
{
	if (accel.Dirty()) UpdateToplevel();
	Synchronize();
	return accel.DebugBvh4( f32Nodes, qNodes, cap );
}

void RenderCore::DebugPoisonTlas( float value )
{
	if (accel.Dirty()) UpdateToplevel();
	Synchronize();
	accel.DebugPoisonTlas( value );
}

void RenderCore::GetAccumulator( float* hostOut4 )
{
	Synchronize();
	CHK_HIP( hipMemcpy( hostOut4, accumulator.ptr, sizeof( float4 ) * (size_t)scrwidth * scrheight, hipMemcpyDeviceToHost ) );
}

void RenderCore::CopyAccumulatorRows( void* devDst, int y0, int y1 )
{
	CHK_HIP( hipMemcpyAsync( devDst, accumulator.ptr + (size_t)y0 * scrwidth, sizeof( float4 ) * (size_t)(y1 - y0) * scrwidth, hipMemcpyDeviceToDevice, stream ) );
	CHK_HIP( hipStreamSynchronize( stream ) );
}

void RenderCore::PackTile( void* devDst, bool ordered, void* consumer )
{
	const int rows = TileRows();
	const int band = tileBand > 0 ? tileBand : std::max( 1, rows ), stride = tileBand > 0 ? tileStride : std::max( 1, rows );
	/* asynchronous: consumers on other streams order themselves after the core stream (lh2_core_stream),
	   so the host can queue the next frame while this one finishes */
	if (!ordered)
	{
		lh2_launch_pack_rows( accumulator.ptr, (float4*)devDst, scrwidth, std::max( 0, tileY0 ), band, stride, rows, {}, stream );
		return;
	}
	/* ordered with a consumer stream (torch's, whose gather reads devDst): the pack waits for the
	   consumer's earlier work on devDst, and the consumer for the pack, through a marker on the
	   consumer stream and the pack launch's own stop event (no marker between the core's kernels);
	   consumer may be the null stream */
	if (!evConsumer) CHK_HIP( hipEventCreateWithFlags( &evConsumer, hipEventDisableTiming ) );
	if (!evPacked) CHK_HIP( hipEventCreate( &evPacked ) );
	CHK_HIP( hipEventRecord( evConsumer, (hipStream_t)consumer ) );
	/* the consumer's earlier work is usually long done (the previous frame's gather): then no wait
	   (a wait packet costs the core stream ~9 us even when its event has completed) */
	if (hipEventQuery( evConsumer ) != hipSuccess) CHK_HIP( hipStreamWaitEvent( stream, evConsumer, 0 ) );
	lh2_launch_pack_rows( accumulator.ptr, (float4*)devDst, scrwidth, std::max( 0, tileY0 ), band, stride, rows, { nullptr, evPacked }, stream );
	CHK_HIP( hipStreamWaitEvent( (hipStream_t)consumer, evPacked, 0 ) );
}

void RenderCore::GetFrame( float* hostOut4 )
{
	Synchronize();
	CHK_HIP( hipMemcpy( hostOut4, frame.ptr, sizeof( float4 ) * (size_t)scrwidth * scrheight, hipMemcpyDeviceToHost ) );
}

/* a unit query over n dense rays; hits non-null: a closest-hit query, traced as the settings "unitCoherent" (as the frame
   traces its tiled primary rays) and "unitTraceWaves" say */
TraceArgs RenderCore::UnitArgs( const float4* o, const float4* d, int n, uint32_t* cursor, int* gstack, uint4* hits ) const
{
	TraceArgs ta{};
	ta.version = TraceVersion();
	ta.rayO = o, ta.rayD = d, ta.countFixed = (uint32_t)n, ta.segStride = (uint32_t)((n + LH2_SEGS - 1) / LH2_SEGS), ta.cursor = cursor;
	ta.hits = hits, ta.gstack = gstack;
	ta.refill = (uint32_t)refillOther, ta.leafBatch = (uint32_t)leafBatch;
	if (hits) ta.packet = unitCoherent && UsePackets() ? 1 : 0, ta.traceWaves = (uint32_t)unitTraceWaves;
	return ta;
}

void RenderCore::TraceClosest( const float* ot, const float* dt, int n, uint32_t* hits4 )
{
	if (accel.Dirty()) UpdateToplevel();
	DevBuf<float4> o, d; DevBuf<uint4> h; DevBuf<int> gs; DevBuf<uint32_t> ovf;
	o.upload( (const float4*)ot, n, stream ), d.upload( (const float4*)dt, n, stream );
	h.resize( n ), ovf.resize( LH2_CURSOR_WORDS );
	gs.resize( (size_t)(LH2_STACK_TOTAL - LH2_STACK_LDS) * TraceGrid() * 256 );
	CHK_HIP( hipMemsetAsync( ovf.ptr, 0, sizeof( uint32_t ) * LH2_CURSOR_WORDS, stream ) );
	const SceneDev sd = MakeSceneDev();
	const TraceArgs ta = UnitArgs( o.ptr, d.ptr, n, ovf.ptr, gs.ptr, h.ptr );
	lh2_launch_trace_closest( &sd, &ta, ta.packet ? PacketGrid() : UnitGrid(), {}, stream );
	CHK_HIP( hipMemcpyAsync( hits4, h.ptr, sizeof( uint4 ) * (size_t)n, hipMemcpyDeviceToHost, stream ) );
	CHK_HIP( hipStreamSynchronize( stream ) );
	CheckSceneError();
}

void RenderCore::TraceAny( const float* ot, const float* dt, int n, uint32_t* occluded )
{
	if (accel.Dirty()) UpdateToplevel();
	DevBuf<float4> o, d; DevBuf<uint32_t> m; DevBuf<int> gs; DevBuf<uint32_t> ovf;
	o.upload( (const float4*)ot, n, stream ), d.upload( (const float4*)dt, n, stream );
	const size_t words = ((size_t)n + 63) / 64 * 2;
	m.resize( words ), ovf.resize( LH2_CURSOR_WORDS );
	gs.resize( (size_t)(LH2_STACK_TOTAL - LH2_STACK_LDS) * TraceGrid() * 256 );
	CHK_HIP( hipMemsetAsync( ovf.ptr, 0, sizeof( uint32_t ) * LH2_CURSOR_WORDS, stream ) );
	CHK_HIP( hipMemsetAsync( m.ptr, 0, words * 4, stream ) );
	const SceneDev sd = MakeSceneDev();
	TraceArgs ta = UnitArgs( o.ptr, d.ptr, n, ovf.ptr, gs.ptr, nullptr );
	ta.mask = m.ptr;
	lh2_launch_trace_any( &sd, &ta, TraceGrid(), 0, {}, stream );
	std::vector<uint32_t> tmp( words );
	CHK_HIP( hipMemcpyAsync( tmp.data(), m.ptr, words * 4, hipMemcpyDeviceToHost, stream ) );
	CHK_HIP( hipStreamSynchronize( stream ) );
	memcpy( occluded, tmp.data(), ((size_t)n + 31) / 32 * 4 );
	CheckSceneError();
}

void RenderCore::TraceClosestDevice( const void* ro, const void* rd, int n, void* hitsOut, int iterations, float* msOut )
{
	if (accel.Dirty()) UpdateToplevel();
	EnsureStack();
	const SceneDev sd = MakeSceneDev();
	DevBuf<uint32_t> cursors;
	cursors.resize( (size_t)std::max( 1, iterations ) * LH2_CURSOR_WORDS );
	CHK_HIP( hipMemsetAsync( cursors.ptr, 0, sizeof( uint32_t ) * (size_t)std::max( 1, iterations ) * LH2_CURSOR_WORDS, stream ) );
#ifdef LH2_TRACE_STATS
	DevBuf<unsigned long long> tstats;
	tstats.resize( LH2_TSTAT_N );
	CHK_HIP( hipMemsetAsync( tstats.ptr, 0, sizeof( unsigned long long ) * LH2_TSTAT_N, stream ) );
#endif
#ifdef LH2_TRACE_TIMES
	DevBuf<unsigned long long> ttimes;
	ttimes.resize( (size_t)std::max( TraceGrid(), PacketGrid() ) * 4 * 4 );
#endif
	/* each launch timed by its own dispatch-recorded start / stop events: msOut is the mean kernel
	   duration, launch gaps excluded (as rocprofv3 --kernel-trace reports it) */
	std::vector<hipEvent_t> ev( 2 * (size_t)std::max( 1, iterations ) );
	for (auto& e : ev) CHK_HIP( hipEventCreate( &e ) );
	for (int i = 0; i < iterations; i++)
	{
		TraceArgs ta = UnitArgs( (const float4*)ro, (const float4*)rd, n, cursors.ptr + (size_t)i * LH2_CURSOR_WORDS, ps.gstack.ptr, (uint4*)hitsOut );
#ifdef LH2_TRACE_STATS
		ta.stats = tstats.ptr;
#endif
#ifdef LH2_TRACE_TIMES
		ta.stats = ttimes.ptr;
#endif
		lh2_launch_trace_closest( &sd, &ta, ta.packet ? PacketGrid() : UnitGrid(), { ev[2 * i], ev[2 * i + 1] }, stream );
	}
	CHK_HIP( hipStreamSynchronize( stream ) );
#ifdef LH2_TRACE_TIMES
	{
		/* the last launch's per-wave times: tools/trace_times.py reads this binary dump */
		std::vector<unsigned long long> h( ttimes.count );
		CHK_HIP( hipMemcpy( h.data(), ttimes.ptr, h.size() * 8, hipMemcpyDeviceToHost ) );
		if (const char* path = getenv( "LH2_TRACE_TIMES_OUT" ))
			if (FILE* f = fopen( path, "wb" )) { fwrite( h.data(), 8, h.size(), f ); fclose( f ); }
	}
#endif
#ifdef LH2_TRACE_STATS
	{
		unsigned long long h[LH2_TSTAT_N];
		CHK_HIP( hipMemcpy( h, tstats.ptr, sizeof( h ), hipMemcpyDeviceToHost ) );
		fprintf( stderr, "LH2_TRACE_STATS {\"rays\": %d, \"launches\": %d, \"c\": [", n, iterations );
		for (int i = 0; i < LH2_TSTAT_N; i++) fprintf( stderr, "%s%llu", i ? ", " : "", h[i] );
		fprintf( stderr, "]}\n" );
	}
#endif
	double total = 0;
	for (int i = 0; i < iterations; i++) { float t = 0; CHK_HIP( hipEventElapsedTime( &t, ev[2 * i], ev[2 * i + 1] ) ); total += t; }
	if (msOut) *msOut = (float)(total / std::max( 1, iterations ));
	CheckSceneError();
	for (auto& e : ev) (void)hipEventDestroy( e );
}

void RenderCore::GenerateEyeRays( const lh2_ViewPyramid& view, uint32_t R0, int pass, float* ot, float* dt, float* st )
{
	const int n = scrwidth * scrheight * scrspp;
	DevBuf<float4> o, d, t4, q4;
	o.resize( n ), d.resize( n ), t4.resize( n ), q4.resize( n );
	CameraParams cp{};
	SetCameraView( cp, view );
	cp.aperture = view.aperture, cp.distortion = view.distortion, cp.geometryEpsilon = geometryEpsilon;
	cp.w = scrwidth, cp.h = scrheight, cp.pass = pass, cp.R0 = R0;
	cp.y0 = 0, cp.tileRows = scrheight, cp.band = scrheight, cp.bandStride = scrheight, cp.tiled = 0, cp.primeRef = primeRef;
	lh2_launch_camera( &cp, dBlueNoise.ptr, o.ptr, d.ptr, t4.ptr, q4.ptr, n, {}, stream );
	std::vector<float4> T( n ), Q( n );
	CHK_HIP( hipMemcpyAsync( ot, o.ptr, sizeof( float4 ) * n, hipMemcpyDeviceToHost, stream ) );
	CHK_HIP( hipMemcpyAsync( dt, d.ptr, sizeof( float4 ) * n, hipMemcpyDeviceToHost, stream ) );
	CHK_HIP( hipMemcpyAsync( T.data(), t4.ptr, sizeof( float4 ) * n, hipMemcpyDeviceToHost, stream ) );
	CHK_HIP( hipMemcpyAsync( Q.data(), q4.ptr, sizeof( float4 ) * n, hipMemcpyDeviceToHost, stream ) );
	CHK_HIP( hipStreamSynchronize( stream ) );
	for (int i = 0; i < n; i++) memcpy( st + i * 8, &T[i], 16 ), memcpy( st + i * 8 + 4, &Q[i], 16 );
}

void RenderCore::SceneInfo( int* nodeCount, int* triCount, int* maxDepth, int* instCount )
{
	if (accel.Dirty()) UpdateToplevel();
	accel.SceneInfo( nodeCount, triCount, maxDepth, instCount );
}

#ifdef LH2_SHADE_TIMES
extern "C" void lh2_shade_times( unsigned long long out[16] );
#endif
void RenderCore::Shutdown()   /* rendercore.cpp:615-650 */
{
	if (!initialized) return;
	(void)hipStreamSynchronize( stream );
#ifdef LH2_SHADE_TIMES
	{
		unsigned long long t[16];
		lh2_shade_times( t );
		fprintf( stderr, "LH2_SHADE_TIMES [" );
		for (int i = 0; i < 16; i++) fprintf( stderr, "%s%llu", i ? ", " : "", t[i] );
		fprintf( stderr, "]\n" );
	}
#endif
	if (aheadStream) (void)hipStreamSynchronize( aheadStream );   /* a TLAS update nothing waited for */
	accel.Shutdown();
	for (auto& e : ps.evTrace) (void)hipEventDestroy( e ), e = nullptr;
	for (auto& e : ps.evShade) (void)hipEventDestroy( e ), e = nullptr;
	for (auto& e : ps.evShadowB) (void)hipEventDestroy( e ), e = nullptr;
	for (auto& e : ps.evCount) (void)hipEventDestroy( e ), e = nullptr;
	for (hipEvent_t* e : { &ps.evCamera, &ps.evShadow, &ps.evSide, &ps.evEarlyEnd }) { if (*e) (void)hipEventDestroy( *e ); *e = nullptr; }
	if (ps.activeLog) (void)hipHostFree( ps.activeLog );
	ps.activeLog = nullptr;
	for (hipEvent_t* e : { &evConsumer, &evPacked }) { if (*e) (void)hipEventDestroy( *e ); *e = nullptr; }
	for (auto& e : fl.ev) { if (e) (void)hipEventDestroy( e ); e = nullptr; }
	for (auto& e : evFrame) (void)hipEventDestroy( e );
	if (glResource) (void)hipGraphicsUnregisterResource( glResource );
	glResource = nullptr, glTexture = 0;
	if (hostStats) (void)hipHostFree( hostStats );
	hostStats = nullptr;
	(void)hipStreamDestroy( stream );
	if (sideStream) (void)hipStreamDestroy( sideStream ), sideStream = nullptr;
	if (aheadStream) (void)hipStreamDestroy( aheadStream ), aheadStream = nullptr;
	stream = nullptr;
	initialized = false;
}

}  // namespace lh2
