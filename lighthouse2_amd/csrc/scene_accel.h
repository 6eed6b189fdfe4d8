/* scene_accel.h - the scene's acceleration structure: meshes, instances, their BLAS and TLAS and the device arrays that hold
   them.  RenderCore owns one and reads it through the few facts a frame needs (the public part below). */
#pragma once
#include <stdint.h>
#include <algorithm>
#include <functional>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/lh2_core_types.h"
#include "bvh_build.h"
#include "bvh_gpu.h"
#include "lh2_kernels.h"
#include "lh2_host.h"

namespace lh2 {

/* the settings that shape a BLAS, used by later SetGeometry calls */
struct BuildSettings
{
	int maxLeaf = 1;
	/* spatial splits (SBVH): overlap threshold x root area; 0 = off.  1e-3 (round 4; 1e-5 before): the same node steps and
	   triangle tests per ray (tools/bvh_quality.cpp: config 2 26.62 / 6.78 vs 26.64 / 6.68, the room 14.58 / 1.83 both)
	   at a third of the build time (config 2 0.39 vs 1.44 s, the room 1.26 vs 2.88 s; profiles/r04d_sbvh_alpha.txt) */
	float spatial = 1e-3f;
	float spatialBudget = 1.0f;          /* ... adding at most this many references per triangle */
	/* ... in nodes of at least this many references (0: every node): 64 builds config 5's 100 meshes 17-20 % faster
	   (setup 4.55 -> 3.64-3.76 s on one box) for 0.3 % more node steps (config-5 frame +0.4 %; config 2 and 3 within the
	   noise), profiles/r04g_sbvh_build.txt, r04u_config5_setup.jsonl */
	int spatialMinRefs = 64;
	int bvh4Collapse = 1;                /* BVH4 collapse: 0 greedy (CollapseBvh4), 1 dynamic programming (CollapseBvh4Sah) */
	int bvh4 = 1;                        /* build BVH4 copies of the BLAS (the default traversal loop needs them) */
	bool operator==( const BuildSettings& o ) const
	{
		return maxLeaf == o.maxLeaf && spatial == o.spatial && spatialBudget == o.spatialBudget && spatialMinRefs == o.spatialMinRefs &&
			bvh4Collapse == o.bvh4Collapse && bvh4 == o.bvh4;
	}
};

/* a deferred CPU BLAS build (SceneAccel::FlushBuilds) and its host results.  Shared by the sub-cores of a MultiDevice:
   the first core to flush runs it (once, std::call_once), every core uploads the results to its own device, and the last
   reference frees them (round 6, VERDICT r5 #7: no N-fold build at deviceCount N) */
struct HostBlas
{
	std::once_flag once;
	BuildSettings settings;              /* what the job builds with: a core shares the build only under the same settings */
	std::function<void( HostBlas&, int )> job;   /* its argument: host threads for the build */
	std::vector<float> nodes2, tris48, nodes4;
	int leafTris = 0, nodeCount = 0, maxDepth = 0, depth4 = 0;
	void Run( int threads );
};

struct CoreMeshHost   /* RenderCore always copies what it needs (rendercore.h:57): all of it on the device */
{
	int triCount = 0;
	int leafTris = 0;                    /* triangle records of the BLAS leaves (> triCount with spatial splits) */
	float aabbLo[3], aabbHi[3];          /* lo.x > hi.x: empty mesh */
	DevBuf<float4> shadeTris;            /* CoreTri4[] in original order, for shading */
	DevBuf<float4> bvhNodes, bvhTris;    /* BLAS with mesh-local refs; relocated into the scene arrays by UpdateToplevel */
	int nodeCount = 0, maxDepth = 0;
	DevBuf<float4> bvh4Nodes;            /* the same BLAS collapsed to BVH4 (CollapseBvh4), mesh-local refs */
	int node4Count = 0, depth4 = 0;
	std::shared_ptr<HostBlas> build;     /* a deferred CPU build not uploaded yet (null: none) */
};

struct CoreInstanceHost { int mesh; float T[16]; float inv[16]; };

class SceneAccel
{
public:
	/* the core stream and the ahead stream (TLAS updates run on it), once; the class creates no stream */
	void Init( hipStream_t core, hipStream_t ahead );
	void Shutdown();
	/* the scene calls of the core ABI (RenderCore forwards them) */
	void SetGeometry( int meshIdx, int triangleCount, const lh2_CoreTri* triangles );
	/* MultiDevice: the same mesh as SetGeometry, sharing src's deferred CPU BLAS build (built once, uploaded here too) */
	void AdoptGeometry( int meshIdx, int triangleCount, const lh2_CoreTri* triangles, const SceneAccel& src );
	void FlushBuilds();
	void SetInstance( int instanceIdx, int meshIdx, const float* matrix16 );
	bool UpdateToplevel();               /* true: the BLAS arrays were laid out anew (new device-resident scene data) */
	void SceneInfo( int* nodeCount, int* triCount, int* maxDepth, int* instCount );
	int DebugBvh4( float* f32Nodes, uint32_t* qNodes, int cap );   /* after the caller's frames have ended */
	void DebugPoisonTlas( float value );                           /* likewise */
	static int BlasBuildCount();         /* CPU BLAS builds run in this process (the build-once check) */

	/* what a frame reads */
	bool Dirty() const { return geometryDirty || instancesDirty; }   /* UpdateToplevel is due */
	void InstancesChanged() { instancesDirty = true; }
	int Slot() const { return tlasSlot; }   /* the latest TLAS slot */
	int* SceneErr( int s ) const { return dSceneError.ptr ? dSceneError.ptr + s : nullptr; }   /* a slot's scene-error word (null before Init) */
	void SyncTlas();                     /* the core stream's next launch reads the latest slot: it waits for that slot's update */
	void ReleaseSlot( int s, hipStream_t st );   /* the last launch reading slot s is queued on st: the slot's next update waits for it */
	/* the latest slot's scene into s (the core stream waits for its update); singleInstanceStart: one instance of a non-empty
	   mesh is entered at its TLAS leaf */
	void Fill( SceneDev& s, bool singleInstanceStart );
	const float* WorldLo() const { return sceneLo; }
	const float* WorldHi() const { return sceneHi; }
	double Bytes() const { return ((double)blasNodeCount + tlasCapacity) * 64.0 + (double)blasTriCount * 48.0; }   /* nodes + triangle records */
	float BuildSeconds() const { return buildSeconds; }   /* host time spent in SetGeometry, AdoptGeometry and FlushBuilds */
#ifdef LH2_TOUCH
	/* diagnostic build: the touched-record bitmap's words, and the records it covers */
	uint32_t TouchNodeWords() const { return (uint32_t)(((size_t)blasNode4Count + 2 * tlasCapacity + 31) / 32); }
	uint32_t TouchTriWords() const { return (uint32_t)(((size_t)blasTriCount + 31) / 32); }
	int Node4Count() const { return blasNode4Count; }
	int TriRecordCount() const { return blasTriCount; }
#endif

	/* settings (RenderCore::Setting) */
	BuildSettings build;
	int buildThreads = 0;                /* host threads of the deferred BLAS builds (setting "buildThreads"; 0: LH2_BUILD_THREADS,
	                                        OMP_NUM_THREADS or min(16, cores)) */
	int gpuBuild = 0, gpuTlas = 1;       /* BLAS builder (1: GPU PLOC, 0: CPU binned SAH); TLAS on the GPU */

private:
	CoreMeshHost& TakeMesh( int meshIdx, int triangleCount, const lh2_CoreTri* triangles );
	void ConcatenateBlas( int instanceCount );
	void BuildBlas4( CoreMeshHost& m, const float* nodes2 );
	hipStream_t stream = nullptr, aheadStream = nullptr;   /* the core's (not owned) */
	float buildSeconds = 0;
	bool pendingBuilds = false;
	std::vector<CoreMeshHost*> meshes;
	std::vector<CoreInstanceHost> instances;
	bool geometryDirty = true, instancesDirty = true;
	DevBuf<float4> dNodes, dTris;
	DevBuf<float4> dNodes4;              /* BVH4: all BLAS (relocated), then the TLAS as two-child nodes */
	DevBuf<uint4> dNodes4q;              /* the same nodes with quantized child boxes (GpuBvhBuilder::Quantize4) */
	DevBuf<uint8_t> dInst[2];            /* DevInstance[], per TLAS slot */
	DevBuf<lh2_CoreInstanceDesc> dInstDesc[2];
	int tlasRoot = 0, blasNodeCount = 0, blasTriCount = 0, blasMeshTris = 0, sceneMaxDepth = 0;   /* blasTriCount: leaf triangle records; blasMeshTris: triangles */
	std::vector<int> meshNodeBase, meshTriBase, meshNode4Base;
	int tlasCapacity = 0, maxBlasDepth = 0;
	int blasNode4Count = 0, maxBlas4Depth = 0;
	/* the 8-wide compressed BVH of round 5 (W8, Ylitie et al. 2017) measured slower in every configuration (its node step
	   issued 1.8x the BVH4 step's VALU for 0.72x the steps: profiles/r05_ab_w8.txt) and was removed in round 6 (commit
	   22e0032 holds it) */
	/* stack entries a ray may need: the BVH2 loop's BLAS depth, the BVH4 loop's 3 per level */
	int StackDepthBound() const { return build.bvh4 ? std::max( maxBlasDepth, 3 * maxBlas4Depth ) : maxBlasDepth; }
	bool tlasOnDevice = false;           /* TLAS of the last UpdateToplevel built by the GPU (depth in dTlasDepth) */
	GpuBvhBuilder gpuBvh;
	DevBuf<float> dMeshBounds;           /* 6 per mesh */
	DevBuf<float> dInstT;                /* 16 per instance */
	DevBuf<int> dInstMesh;
	DevBuf<int> dSceneError, dTlasDepth; /* dSceneError: one flag per TLAS slot */
	DevBuf<int> dBlasQError;             /* the BLAS quantizer's range flag (LH2_SCENE_ERR_QRANGE), copied into dSceneError per TLAS update */
	uint8_t* stage[2] = {};              /* pinned staging of UpdateToplevel (double-buffered) */
	size_t stageBytes[2] = {};
	hipEvent_t evStage[2] = {};
	int stageSlot = 0;
	/* TLAS slots (round 4): an instance-only UpdateToplevel writes the instance tables, the TLAS (the BVH2 and BVH4 regions
	   after the BLAS, tlasCapacity nodes per slot) and the scene-error flag of the slot no frame in flight reads, on the ahead
	   stream behind the last frame that read that slot (evTlasFree), so an animated frame's primary launch can still run
	   beside the previous frame; the core stream waits for the update (evTlasReady) before its next launch */
	int tlasSlot = 0;
	int tlasNodeCount[2] = { 1, 1 };     /* the nodes of each slot's TLAS (UpdateToplevel) */
	bool tlasPending = false, tlasFreeValid[2] = {};
	hipEvent_t evTlasReady = nullptr, evTlasFree[2] = {};
	int TlasBase2( int s ) const { return blasNodeCount + s * tlasCapacity; }
	int TlasBase4( int s ) const { return blasNode4Count + s * tlasCapacity; }
	float sceneLo[3] = { 0, 0, 0 }, sceneHi[3] = { 0, 0, 0 };   /* world box of the instanced meshes (UpdateToplevel) */
	float qBound = 0;                    /* |coordinate| bound of the world box and every mesh box, with slack (SceneDev::qBound) */
};

}  // namespace lh2
