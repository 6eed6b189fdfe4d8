/* rendercore.h - host side of the MI355X render core (counterpart of
   RenderCore_OptixPrime_B/rendercore.h:48-142; same method names and call contract). */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/lh2_core_types.h"
#include "../../include/lh2_rendercore.h"
#include "lh2_kernels.h"
#include "lh2_filter.h"
#include "lh2_device.h"
#include "scene_accel.h"

namespace lh2 {

/* one set of path buffers: rays, path state and hits.  A launch reads one set and (a shade launch) writes another */
struct PathSet
{
	float4 *O, *D, *T4, *Q4;
	uint4* hits;
	void Rays( TraceArgs& a ) const { a.rayO = O, a.rayD = D, a.hits = hits; }
	void In( ShadeParams& p ) const { p.rayO = O, p.rayD = D, p.T4 = T4, p.Q4 = Q4, p.hits = hits; }
	void Out( ShadeParams& p ) const { p.rayOut = O, p.rayDOut = D, p.T4Out = T4, p.Q4Out = Q4; }
};

/* what the launches of one frame parity own (PathStreams: "per frame parity") */
struct FrameSlots
{
	Counters* c;
	uint32_t *cursors, *rayLog;
	float4 *shO, *shD, *shP;
	uint32_t *shMask, *shSnap;           /* shSnap: the shadow rays queued before the path tail */
	float4* delta;
	uint32_t* Cursor( int slot ) const { return cursors + (size_t)slot * LH2_CURSOR_WORDS; }   /* a launch's work-queue heads (LH2_CURSOR_SLOTS) */
};

/* the frame's path and ray streams (segmented, lh2_kernels.h) with their counters, work-queue heads,
   traversal stacks and the events that time the frame's launches.  Buffers, events and the state that crosses frames
   (marked "crosses frames"); what Synchronize needs to know about the last frame is RenderCore::last */
struct PathStreams
{
	size_t cap = 0;                      /* paths the buffers hold */
	DevBuf<float4> rayO[2], rayD[2], T4[2], Q4[2];
	DevBuf<uint4> hits;
	/* the primary rays, path state and hits of a fused frame (k_trace_primary_packet writes them, its first shade
	   launch reads them): apart from the bounce ping-pong, so the next frame's primary launch can run beside this
	   frame's later bounces */
	DevBuf<float4> rayOP[2], rayDP[2], T4P[2], Q4P[2];   /* per frame parity */
	DevBuf<uint4> hitsP[2];
	PathSet Bounce( int i ) const { return { rayO[i].ptr, rayD[i].ptr, T4[i].ptr, Q4[i].ptr, hits.ptr }; }
	PathSet Primary( int parity ) const { return { rayOP[parity].ptr, rayDP[parity].ptr, T4P[parity].ptr, Q4P[parity].ptr, hitsP[parity].ptr }; }
	DevBuf<float4> shO, shD, shP;        /* 2 x shCap (frame parity) */
	DevBuf<uint32_t> shMask;             /* 2 x shMaskWords */
	size_t shCap = 0, shMaskWords = 0;
	DevBuf<int> gstack;
	DevBuf<int> sideStack;               /* the side shadow launch's global stack (shadowOverlap) */
	DevBuf<int> aheadStack;              /* a per-ray primary launch beside the previous frame (RenderCore::kCamAhead) */
	DevBuf<uint32_t> shSnap;             /* the shadow rays queued before the path tail, per segment (advance_bounce), per frame parity */
	/* per frame parity (fp): two consecutive frames' counters, work-queue heads, shadow streams and ray-count logs are
	   apart, so the next frame's first launches can run beside this frame's last ones (frame overlap, early shade) */
	DevBuf<Counters> counters;           /* 2 */
	DevBuf<uint32_t> cursors;            /* 2 x LH2_CURSOR_SLOTS x LH2_CURSOR_WORDS work-queue heads */
	DevBuf<uint32_t> rayLog;             /* 2 x LH2_RAYLOG */
	DevBuf<uint32_t> hv;                 /* heavy-first packets: two blocks (TraceArgs::hvRead / hvWrite), the frame parity picks */
	uint32_t hvCap = 0, hvMaskWords = 0, hvBlock = 0;
	uint32_t hvParity = 0;               /* crosses frames: the block the next frame's packets read */
	uint32_t* activeLog = nullptr;       /* pinned: extension rays after each bounce (advance_bounce) */
	/* a launch carries only a stop event (a start event costs its dispatch ~5 us of idle GPU); a timed
	   interval runs from the previous launch's stop event, so it includes the launch gap */
	hipEvent_t evTrace[LH2_MAX_BOUNCES + 1] = {}, evShade[LH2_MAX_BOUNCES + 1] = {}, evShadowB[LH2_MAX_BOUNCES + 1] = {};
	hipEvent_t evCount[LH2_MAX_BOUNCES + 2] = {}, evCamera = nullptr, evShadow = nullptr;
	hipEvent_t evSide = nullptr, fromSide = nullptr;   /* shadowOverlap: the side launch */
	hipEvent_t countReady[LH2_MAX_BOUNCES + 2] = {};   /* [L]: the event after which bounce L's hand-off is done (evShade or evCount, not owned) */
	hipEvent_t fromTrace[LH2_MAX_BOUNCES + 1] = {}, fromShade[LH2_MAX_BOUNCES + 1] = {}, fromShadowB[LH2_MAX_BOUNCES + 1] = {}, fromShadow = nullptr;
	hipEvent_t prevStop = nullptr;       /* the stop event of the frame's last timed launch so far */
	/* a launch with stop event `stop` was queued: its timed interval starts at the previous launch's stop event */
	void Stamp( hipEvent_t& from, hipEvent_t stop ) { from = prevStop, prevStop = stop; }
	/* the stream layout of the frame being rendered (after Render: the last frame's) */
	uint32_t count = 0, segStride = 0, shadowStride = 0;
	int fp = 0;                          /* its parity */
	/* crosses frames.  The camera fused into the primary packet launch (setting "cameraFused"): the heavy-packet block the
	   next frame records into is zeroed by the frame's first shade launch (hvNextZeroed: it was) */
	bool hvNextZeroed = false;
	/* crosses frames.  Frame overlap (setting "frameOverlap"): the primary launch of a fused frame runs on the ahead stream
	   after the previous frame's first shade launch, unless something since then needs it to wait for the whole previous
	   frame (relaid: buffers were reallocated or the last frame was filtered) */
	bool lastFused = false, relaid = true;
	uint64_t lastSceneVersion = 0;
	hipEvent_t overlapEv = nullptr;      /* the last frame's shade launch the next primary launch waits for (not owned) */
	hipEvent_t evEarlyEnd = nullptr;     /* an early frame that ended before its path tail: overlapEv on the core stream (owned) */
	/* crosses frames.  Early shade (setting "earlyShade"): the next frame's first shade launch also runs beside this frame's
	   launches after overlapEv.  Those use one ping-pong buffer (busy: the path tail's, or the last bounce's rays) and write
	   neither (earlyOk), so the next frame's first shade writes the other one */
	int busy = 0;
	bool earlyOk = false;
};

/* every decision Render makes before it queues anything (RenderCore::PlanFrame): constant for the rest of the frame */
struct FramePlan
{
	bool restart, filt;                  /* the accumulation starts over; the denoise mode runs this frame */
	bool taa;                            /* ... and ends in the TAA stage (setting "TAA") */
	int tileRows;
	uint32_t pathCount, segStride;
	float aperture;
	int maxPL, tailL;                    /* bounces at most; the path-tail launch (pathLength), 0: none */
	bool packets;                        /* the primary rays are traced as packets */
	bool fusedCam, camAhead;             /* the camera fused into the primary packet launch; camera + per-ray primary launch apart */
	bool pFrame;                         /* either: the primary stage has buffers of its own and may run beside the previous frame */
	bool serialize;                      /* ... but runs behind it, on the core stream, this frame */
	bool early;                          /* the first shade launch follows the primary launch on the ahead stream */
	bool clearAll, clearByLaunch, clearBehind;   /* how a restart zeroes the accumulator (PlanFrame, BeginFrame) */
	bool growPaths;                      /* BeginFrame is about to reallocate the path buffers */
	bool hvOn, hvRelayout;               /* heavy-first primary packets; their blocks are (re)allocated first */
	uint32_t hvCap, hvTiles;
	float hvFactor;
	bool small;                          /* at most kSmallFramePaths paths */
	bool shadows, overlap;               /* the scene has lights; the shadow rays before the tail go to the side stream */
	bool bounceShadows, finalShadows, handOffLaunch;   /* PrimeRef's launches after every bounce, or one shadow launch per frame */
	bool terminal;                       /* ShadeParams::terminal of the bounces past the first */
	bool besideNext;                     /* the next frame's primary launch will likely run beside this frame's launches after ... */
	int overlapL;                        /* ... the shade launch of this bounce, the next frame's overlap event */
	int traceWaves;
	uint32_t tailWaves;
	int traceGrid, closestGrid, besideGrid, primaryGrid, shadeGrid, tailGrid, sideGrid, finalShadowGrid;
};

/* what Synchronize, GetRayCounts and GetCoreStats read about the last rendered frame (written once, at the end of Render) */
struct LastFrame
{
	int pl = 0;                          /* bounces launched */
	int tailL = 0;                       /* its path-tail launch (pathLength), 0: none */
	int pathLengths = 0;                 /* path lengths with a ray count (a path tail: all of them) */
	bool early = false, sideOn = false;  /* its first shade launch ran early; its early shadow rays on the side stream */
	bool shadows = true, primeRef = false, filtered = false, overlapped = false;
	bool taa = false;                    /* a filtered frame that ended in the TAA stage */
};

struct Frame;   /* a frame being queued (rendercore.cpp) */

/* the denoise mode's buffers (setting "filter"; lh2_filter.h), allocated only while it is on.  Index cur: the frame being
   rendered (after Render: the last frame's); 1 - cur: the frame before it */
struct FilterState
{
	DevBuf<uint4> features;
	DevBuf<float4> worldPos[2], moments[2], deltaDepth, shading;
	DevBuf<float2> motion;
	DevBuf<float4> filtered[2];          /* [cur]: the frame's phase-1 output (the next frame's history); [1 - cur]: phase 2's */
	/* setting "TAA", allocated only while it and the filter are applied: the last pass's linear output, and the TAA pass's
	   pixels ([cur]: this frame's, the next frame's history) */
	DevBuf<float4> linear, taa[2];
	size_t taaPixels = 0;                /* what they hold (0: not allocated) */
	bool taaValid = false;               /* taa[1 - cur] holds the previous frame's pixels, if historyValid says there was one */
	int cur = 0;
	size_t pixels = 0;                   /* what the buffers hold (0: not allocated) */
	bool historyValid = false;           /* the buffers of 1 - cur hold the previous frame */
	lh2_ViewPyramid prevView{};
	hipEvent_t ev[7] = {};               /* the chain's start, and the stop events of prepare, the three passes, the TAA pass and the unsharpen */
	float ms[6] = {};                    /* the last filtered frame's kernel times (ms); [4], [5]: the TAA stage's, 0 without it */
};

struct FrameStats   /* per-frame values delivered by k_finalize into pinned host memory */
{
	uint32_t rayCount[LH2_MAX_BOUNCES + 1];
	Counters counters;
	int sceneError;
};

class RenderCore
{
public:
	void Init();
	void SetProbePos( int x, int y ) { probeX = x, probeY = y; }
	void SetTarget( uint32_t w, uint32_t h, uint32_t spp );
	void SetInteropTexture( uint32_t glTextureId );   /* 0: headless (frame stays in the device buffer) */
	void Setting( const char* name, float value );
	bool GetSetting( const char* name, float& value ) const;
	void Render( const lh2_ViewPyramid& view, int converge );
	void Shutdown();
	void SetTextures( const lh2_CoreTexDesc* tex, int textureCount );
	void SetMaterials( const lh2_CoreMaterial* mat, int materialCount );
	void SetLights( const lh2_CoreLightTri* areaLights, int areaLightCount, const lh2_CorePointLight* pointLights, int pointLightCount,
		const lh2_CoreSpotLight* spotLights, int spotLightCount, const lh2_CoreDirectionalLight* directionalLights, int directionalLightCount );
	void SetSkyData( const float* pixels, uint32_t width, uint32_t height );
	void SetGeometry( int meshIdx, const float* vertexData, int vertexCount, int triangleCount, const lh2_CoreTri* triangles, const uint32_t* alphaFlags );
	/* MultiDevice: the same mesh as SetGeometry, sharing src's deferred CPU BLAS build (built once, uploaded here too) */
	void AdoptGeometry( int meshIdx, int triangleCount, const lh2_CoreTri* triangles, const RenderCore& src );
	void FlushPendingBuilds() { accel.FlushBuilds(); }
	static int BlasBuildCount() { return SceneAccel::BlasBuildCount(); }   /* CPU BLAS builds run in this process (the build-once check) */
	void SetInstance( int instanceIdx, int meshIdx, const float* matrix16 ) { accel.SetInstance( instanceIdx, meshIdx, matrix16 ); }
	void UpdateToplevel();
	lh2_CoreStats GetCoreStats();

	/* extensions beyond the reference ABI (tile partition, headless output, unit-level kernels) */
	void SetTile( int y0, int y1 ) { tileY0 = y0, tileY1 = y1, tileBand = 0, tileStride = 0, tileChanged = true; }
	/* rank r of n owns the row bands [r*band + k*n*band, +band): balanced multi-GPU partition */
	void SetTileBands( int rank, int nranks, int band ) { tileY0 = rank * band, tileY1 = -1, tileBand = band, tileStride = nranks * band, tileChanged = true; }
	int TileRows() const;
	void Synchronize();
	void GetAccumulator( float* hostOut4 );                /* full frame, raw accumulator */
	void CopyAccumulatorRows( void* devDst, int y0, int y1 ); /* D2D copy of rows [y0,y1) */
	void PackTile( void* devDst, bool ordered = false, void* consumer = nullptr );   /* owned rows, local order (async); ordered: with the stream consumer (null: the null stream) both ways */
	hipEvent_t evConsumer = nullptr, evPacked = nullptr;
	void GetFrame( float* hostOut4 );                      /* finalizeRender output: acc / samplesTaken */
	/* the denoise mode (setting "filter"): its buffers of the last frame, to the host (LH2_FILTER_BUF_*, lh2_rendercore.h),
	   the last frame's kernel times, and a unit entry that runs prepare (stage 0) or one a-trous pass (stage 1 .. 3) on host arrays */
	void GetFilterBuffer( int which, void* hostOut );
	void GetFilterTimes( float* ms4 );
	void FilterUnit( const lh2_FilterUnit& u );
	/* the TAA stage (setting "TAA"): the last frame's two kernel times (zeros if it ran none), and its unit entry */
	void GetTaaTimes( float* ms2 );
	void TaaUnit( const lh2_TaaUnit& u );
	void BsdfUnit( const lh2_BsdfUnit& u );
	void SetFilterAllowed( bool on );    /* MultiDevice: a band has no neighbours across its edge, so no core of it filters */
	bool FilterOn() const { return filterOn && filterAllowed; }
	bool TaaOn() const { return taaOn && FilterOn(); }   /* applied only where the filter is */
	/* in-process multi-device gather (multidevice.cpp): rows packed by the core of rank `rank` of a
	   band partition, already on this device, into this accumulator (async); then the frame output
	   of the whole accumulator again (finalizeRender + display copy, no statistics) */
	void UnpackTile( const void* devSrc, int rank, int nranks, int band );
	void FinalizeFrame();
	bool displayAtFinalize = false;   /* rank 0 of MultiDevice: the display copy follows the gather (FinalizeFrame) */
	void CopyFrameAsync( void* devDst );   /* the last finalized frame, D2D on the core stream */
	hipStream_t Stream() const { return stream; }
	int Device() const { return device; }
	int SamplesTaken() const { return samplesTaken; }
	void GetRayCounts( uint32_t* out17 );
	/* diagnostics: the last frame's queued shadow rays {O, tmin} {D, tmax} {potential rgb, pixel bits}, segment by segment */
	int DebugShadowRays( float* o4, float* d4, float* p4, int cap );
	int DebugBvh4( float* f32Nodes, uint32_t* qNodes, int cap );   /* the BVH4 nodes, f32 (32 floats) and quantized (16 words) */
	void DebugPoisonTlas( float value );   /* test hook: both TLAS slots' node regions filled with value */
	void TraceClosest( const float* orgTmin4, const float* dirTmax4, int n, uint32_t* hits4 );   /* host in/out */
	void TraceAny( const float* orgTmin4, const float* dirTmax4, int n, uint32_t* occluded );
	void TraceClosestDevice( const void* rayO, const void* rayD, int n, void* hits, int iterations, float* msOut );
	void GenerateEyeRays( const lh2_ViewPyramid& view, uint32_t R0, int pass, float* orgTmin4, float* dirTmax4, float* state8 );
	void SceneInfo( int* nodeCount, int* triCount, int* maxDepth, int* instCount );
	float lastKernelMs[8] = {};  /* traceTime of the last frame per bounce (diagnostics) */

	lh2_CoreStats coreStats{};
	hipStream_t stream = nullptr;
	hipStream_t sideStream = nullptr;    /* shadowOverlap: the device's least priority (the default level on MI355X) */
	hipStream_t aheadStream = nullptr;   /* frameOverlap: the fused primary launch */

private:
	void EnsureBuffers();
	void EnsureFilterBuffers();
	void RunFilter( const lh2_ViewPyramid& view, bool taa );
	void EnsureTaaBuffers();
	void FreeTaaBuffers();
	bool filterOn = false, filterAllowed = true;
	bool taaOn = false;                  /* the setting as sent; TaaOn(): applied */
	int filterLds = -1;                  /* the a-trous passes' taps from an LDS tile (1), through L1 / L2 (0); -1: the measured pick per pass */
	float clampDirect = LH2_FILTER_CLAMP_DIRECT, clampIndirect = LH2_FILTER_CLAMP_INDIRECT;
	FilterState fl;
	/* the a-trous passes' tap source per pass (1: an LDS tile), by measurement (profiles/ *_ab_filter_lds.txt) */
	static constexpr int kFilterLdsPick[3] = { 1, 1, 1 };
	/* the same for the TAA pass (profiles/ *_ab_taa_lds.txt; the unsharpen has one variant) */
	static constexpr int kTaaLdsPick = 1;
#ifdef LH2_TOUCH
	DevBuf<uint32_t> touchMap;           /* diagnostic build: the touched-record bitmap (lh2_trace4d.inc) */
	uint32_t touchNodeWords = 0;
	void TouchBegin();
	void TouchReport( int pathLength );
#endif
	bool PathsFit( uint32_t paths ) const { return (size_t)paths + 64 <= ps.cap; }
	void EnsurePaths( uint32_t paths );
	void EnsureStack();
	/* Render's steps: the plan (no HIP call), the state transitions and buffers, then the launch stages */
	FramePlan PlanFrame( const lh2_ViewPyramid& view, int converge ) const;
	void BeginFrame( Frame& f, int converge );
	void PrimaryStage( Frame& f );
	void BounceLoop( Frame& f );
	void TraceBounce( Frame& f, int pathLength );
	void ShadeBounce( Frame& f, int pathLength );
	void PathTail( Frame& f, int pathLength );
	void FinalShadows( Frame& f );
	void FinishFrame( Frame& f );
	void CopyFrameToDisplay();
	void LaunchClosest( const Frame& f, const TraceArgs& ta, int grid, int pathLength, hipStream_t st );   /* stop event: evTrace[pathLength] */
	TraceArgs BounceArgs( const Frame& f, int pathLength, const PathSet& rays ) const;
	ShadeParams ShadeArgs( const Frame& f, int pathLength ) const;
	BounceAdvance HandOff( const Frame& f, int pathLength ) const;
	TraceArgs ShadowArgs( const FrameSlots& s, const uint32_t* segCounts, int cursorSlot, int leafBatch, int* gstack ) const;
	TraceArgs UnitArgs( const float4* o, const float4* d, int n, uint32_t* cursor, int* gstack, uint4* hits ) const;
	void CheckSceneError();
	bool UsePackets() const;
	SceneDev MakeSceneDev();             /* the latest TLAS slot's scene; the core stream waits for its update (SceneAccel::Fill) */
	FrameSlots Slots() const;            /* of the frame parity PathStreams::fp */
	int TraceGrid() const { return smCount * blocksPerCU; }
	int UnitGrid() const { return smCount * std::min( blocksPerCU, unitTraceWaves == 8 ? traceBlocksPerCU8 : traceBlocksPerCU7 ); }
	int PacketGrid() const { return smCount * packetBlocksPerCU; }   /* packet kernel: its own occupancy */
	int PathGrid() const { return smCount * std::min( blocksPerCU, pathBlocksPerCU ); }   /* path tail: its occupancy, within the stack's */

	int device = 0, smCount = 256, blocksPerCU = 8, maxBlocksPerCU = 8, packetBlocksPerCU = 8, pathBlocksPerCU = 3, pathBlocksPerCU4 = 4;
	int traceBlocksPerCU7 = 7, traceBlocksPerCU8 = 8;   /* occupancy of the closest-hit kernel's 7- and 8-wave variants */
	/* closest-hit launches with the chip alone: 0, the 7-wave variant (72 VGPRs); 7 or 8: that variant.  8 for every scene won
	   in round 4; with the early node loads (round 5: single-instance loops only) the single-instance 8-wave loop spills, and 7
	   there is config 3 -3.4 %, 4K -3 %, the N = 8 share -2.9 % (profiles/r05f_ab_trace_waves.txt); round 6 gave the instanced
	   loops the early loads too, at 7 waves (config 5 9.31-9.32 -> 9.19-9.21 ms; at 8 they spill: 13.2 ms,
	   profiles/r06l_ab_instanced_early.txt) */
	int traceWaves = 0;
	int userBlocksPerCU = 0;             /* setting "traceBlocksPerCU" (0: not set) */
	/* the closest-hit kernel variant a per-ray launch with the chip alone takes (traceWaves 0: 7), and its grid's
	   blocks per CU: the variant's occupancy, or the user's setting within it */
	int ScenePicksWaves() const { return traceWaves ? traceWaves : 7; }
	int ClosestBlocksPerCU( int waves ) const
	{
		const int occ = waves == 7 ? traceBlocksPerCU7 : traceBlocksPerCU8;
		return userBlocksPerCU ? std::min( userBlocksPerCU, occ ) : occ;
	}
	int unitTraceWaves = 7;              /* the unit queries' variant: 7 (the config-2 bounce rays alone: 0.481 vs 0.515 ms, r04ag) */
	bool initialized = false;
	SceneAccel accel;                    /* the scene: meshes, instances, BLAS, TLAS slots and their device arrays */
	hipGraphicsResource_t glResource = nullptr;   /* registered GL_RGBA32F target texture */
	uint32_t glTexture = 0;
	DevBuf<uint4> dMaterials;
	int materialCount = 0;               /* the records SetMaterials uploaded (BsdfUnit checks its indices against it) */
	std::vector<lh2_CoreTexDesc> texDescs;   /* copies, firstPixel assigned per storage (rendercore.cpp:276-292) */
	DevBuf<uint32_t> dArgb32, dNrm32;        /* continuous texel arrays (rendercore.cpp:299-336) */
	DevBuf<float4> dArgb128;
	DevBuf<lh2_CoreLightTri> dArea; DevBuf<lh2_CorePointLight> dPoint; DevBuf<lh2_CoreSpotLight> dSpot; DevBuf<lh2_CoreDirectionalLight> dDir;
	int nArea = 0, nPoint = 0, nSpot = 0, nDir = 0;
	DevBuf<float> dSky; int skyW = 0, skyH = 0;
	DevBuf<uint8_t> dBlueNoise;
	/* settings (rendercore.h DeviceVars; constant-memory defaults: .cuda.cu:38-39) */
	float geometryEpsilon = 0.0f, clampValue = 10.0f;
	int maxPathLength = 16;
	bool diffuseOnly = false;            /* SetMaterials: no material can continue a path past its second vertex */
	bool canEmit = true;                 /* SetMaterials: some material may shade as emissive (colour > 1 or colour maps) or cut out */
	int primeRef = 0;                    /* RenderCore_PrimeRef validation mode (setting "primeRef") */
	int probeX = 0, probeY = 0;
	/* target + frame buffers */
	int scrwidth = 0, scrheight = 0, scrspp = 1;
	int tileY0 = 0, tileY1 = -1, tileBand = 0, tileStride = 0;
	DevBuf<float4> accumulator, frame;
	DevBuf<float4> delta;                /* early shade: the first shade launch's accumulator additions (FrameStatsDev::delta), per frame parity */
	PathStreams ps;                      /* on `stream`; also serves the unit-level trace calls */
	bool tileChanged = false;            /* the next restart clears the whole accumulator, not only the tile's pixels */
	LastFrame last;
	bool singleInstanceStart = true;     /* one instance of a non-empty mesh: rays start at its TLAS leaf (SceneDev::tlasRoot) */
	bool terminalShade = true;           /* k_shade<true> for shade passes whose hits cannot contribute (ShadeParams::terminal) */
	FrameStats* hostStats = nullptr;     /* pinned */
	bool statsPending = false;
	hipEvent_t evFrame[3] = {};          /* the frame's start marker, its end (finalize), the previous frame's end */
	bool frameEndRecorded = false, prevFrameEndValid = false;
	int tiledRays = 1;                   /* primary rays stored in 8x8 pixel blocks per wave (coherent packets) */
	int cameraFused = 1;                 /* primary rays made by the packet launch itself (k_trace_primary_packet), no camera launch */
	/* a fused frame's primary launch beside the previous frame's later bounces (aheadStream): 1, after its shade launch
	   before the path tail (its first without one); 2, after its first shade launch; 0: off.  Right after the previous
	   frame's primary launch, beside its first shade launch too, measured slower (profiles/r05_ab_frame_overlap_chain.txt) */
	int frameOverlap = 1;
	/* with frameOverlap 1: the next frame's first shade launch follows its primary launch on the ahead stream, beside this
	   frame's path tail and shadow launches, instead of after them on the core stream (frames whose later launches use one
	   ping-pong buffer: PathStreams::earlyOk).  Accumulator additions of the two frames then interleave: the sum matches
	   the sequential one within float rounding, not bit for bit (the first-vertex depths, w, stay exact) */
	int earlyShade = 1;
	/* fixed policy constants (round 5: the knobs behind them were pruned; the values are the measured winners).
	   Small frames (at most kSmallFramePaths paths: the N = 8 rank share, config 3) take the early shade (beside a large frame's
	   tail it gains nothing and its fold costs: config-4 N = 1 1 % slower, r04e_ab.txt) and the path tail at 3 blocks per CU
	   beside the side shadow launch (large frames 2: the 4K frame 6.54 vs 6.64-6.69 ms, r04p_ab.txt, r04r_ab.txt) */
	static constexpr float kSmallFramePaths = 2.5e6f;
	/* the shade launches' grid: about kShadePathsPerThread paths per thread, between the trace grid and kShadeMaxBlocks per CU
	   (the N = 8 share 12 blocks per CU, config 3 24: -1.5 / -1.5 %, r04al_ab.txt, r04am_ab.txt, r04av_ab.txt) */
	static constexpr float kShadePathsPerThread = 1.3f;
	static constexpr int kShadeMaxBlocks = 24;
	/* blocks per CU of a closest-hit launch that the next frame's primary launch runs beside (an overlapped frame's later
	   bounces, no path tail): the packets' latency-bound waves get slots from the start (config 2 +4 %, r03q_ab_trace_blocks.txt) */
#ifndef LH2_OVERLAP_TRACE_BLOCKS
#define LH2_OVERLAP_TRACE_BLOCKS 5
#endif
	static constexpr int kOverlapTraceBlocks = LH2_OVERLAP_TRACE_BLOCKS;
	/* packets while the BVH + triangles fit the 256 MB Infinity Cache (a packet's node and triangle records come through
	   the scalar cache, one at a time: beyond the cache each is a DRAM round trip).  Config 3 (134 MB): primary 0.29 ->
	   0.24 ms with packets; config 5 (1.4 GB): 5.3 -> 7.8 ms (profiles/r02zc_ab_packets_configs.txt) */
	static constexpr double kPacketMaxBytes = 256.0 * 1048576.0;
	uint64_t sceneVersion = 0;           /* incremented by every change of device-resident scene data or buffers */
	/* dynamic ray fetch: refill a wave's idle lanes once this many are idle; BLAS leaves parked until this many
	   lanes hold one (lh2_trace4d.inc).  Primary rays: coherent 8x8-tiled batches (profiles/r01c_sweep_bvh4.jsonl,
	   r02y_ab_v7.txt); leafBatch 8 with the quantized nodes (bounce 0.492 -> 0.488 ms, N = 8 share 1.35 -> 1.32 ms,
	   r03k_ab_leafbatch.txt) */
	int refillOther = 48, leafBatch = 8;   /* primary rays traced per ray (no packets) take the same (profiles/r04ag_refill_sweep.txt;
	                                          round 5: 32 / 40 / 56 no better, r05f_ab_refill.txt, r05f_ab_beside_refill.txt) */
	/* the shadow launches park BLAS leaves until 16 lanes hold one (the closest-hit launches: leafBatch): config 3 -0.4 %, the
	   4K frame -0.9 %, the N = 8 share -0.3 % against 8; 2 and 4 slower, 24 no better; their refill stays refillOther (32 and
	   60 slower) (profiles/r05f_ab_lazy_frame_shadow_sweep.txt, r05f_ab_shadow_leafbatch.txt) */
	static constexpr int kShadowLeafBatch = 16;
	/* the primary launch's work-queue heads: bounce 1's slot of the frame parity's block, left alone by the launch's own resets
	   and zeroed by the finalize of the frame before the previous one (FrameStatsDev::zeroHeads) */
	static constexpr int kPrimarySlot = 1;
#ifndef LH2_CAM_AHEAD
#define LH2_CAM_AHEAD 1
#endif
	/* frames traced per ray (no packets) overlap like packet frames: camera + per-ray primary launch on the ahead stream
	   (config 5 9.70-9.73 -> 9.48-9.51 ms, profiles/r06b_ab_cam_ahead.txt); the touch build counts one closest-hit launch at a
	   time (TouchReport), so it keeps them behind the previous frame */
#ifdef LH2_TOUCH
	static constexpr bool kCamAhead = false;
#else
	static constexpr bool kCamAhead = LH2_CAM_AHEAD != 0;
#endif
	float chordSplit = 0.35f;            /* extension rays with a chord through the scene box below this x its extent are traced last */
	/* the path tail (k_trace_path4d): bounces pathTail .. maxPathLength traced and shaded in one launch,
	   a wave shading its finished queries once pathTailBatch lanes hold one (or none walks); 0: a launch
	   pair per bounce.  Config 3 (profiles/r02zb_ab_path_tail.txt): 2.542 -> 2.389 ms per frame at 3 / 56 */
	int pathTail = 3, pathTailBatch = 56;
	/* shadow overlap: the shadow rays queued before the path tail are traced on a side stream
	   while the path tail runs (latency bound, it leaves much of the chip idle); the final shadow launch
	   traces only the path tail's.  Config 3 2.29 -> 2.235 ms, config-4 rank share at N = 8 1.431 -> 1.363
	   ms with the tail at 2 blocks per CU (profiles/r03g_overlap_sweep.txt); a side launch after every
	   shade launch slows the bounces it overlaps (2.344 / 1.426 ms) */
	bool shadowOverlap = true;
	int pathTailBlocks = 0;              /* the path tail's blocks per CU; 0: with the overlap 3 for frames of at most
	                                        kSmallFramePaths paths, else 2 (without: its occupancy limit) */
	/* the path tail kernel's variant: 0, by frame size (3 waves per SIMD for small frames, 4 for larger ones); 3 or 4 */
	int pathTailWaves = 0;
	/* blocks per CU of the frame's last shadow launch (0: the trace grid's): fewer leave the next frame's primary and early
	   shade launches room beside it: 6 against the trace grid's 8, config 3 and the N = 8 share -0.5 % (profiles/r04aj_ab.txt,
	   r04ak_ab.txt); round 5, with the shorter shade launches, 4 against 6: the N = 8 share -0.9 %, config 3 -0.3 %, 8 slower
	   (r05f_ab_final_shadow_blocks.txt) */
	int finalShadowBlocks = 4;
	int shadeBlocks = 0;                 /* blocks per CU of the frame's shade launches (0: by path count, Render) */
	/* blocks per CU of the side shadow launch beside the path tail (0: the trace grid's; -1: by frame size): 4 leaves the next
	   frame's primary and early shade launches room: config 3 -0.5 %, the N = 8 share -0.8 to -1.5 % (profiles/r04m_ab.txt,
	   r04n_ab.txt); round 6, with the lighter 4-wave path tail, small frames (<= kSmallFramePaths) 3: config 3 -1.2 %, the N = 8
	   share -1.8 %, while the 4K frame stays at 4 (3 there: +2 %, profiles/r06y_ab_side_blocks.txt) */
	int sideBlocks = -1;
	/* heavy-first primary packets (TraceArgs::hvRead): the packets of the previous frame that took more than
	   packetHeavy x its mean node steps are taken first; 0: off; -1 (default, round 6): 3 for frames with a path tail, whose
	   primary launch runs beside the previous frame's tail (config 3 -1.2 %, the 4K frame -0.8 %), 2 otherwise (config 2: 3
	   is 1.5 % slower), profiles/r06zg_ab_overlap_heavy.txt */
	float packetHeavy = -1.0f;
	int traceVersion = 0;                /* 0: auto (TraceVersion) */
	int TraceVersion() const;
	int unitCoherent = 0;
	int packetPrimary = -1;              /* wave-uniform packet traversal for 8x8-tiled primary rays (-1: by scene size) */
	double frameHostMs = 0;
	int samplesTaken = 0;
	bool firstConvergingFrame = false;
	uint32_t camRNGseed = 0x12345678;
};

}  // namespace lh2
