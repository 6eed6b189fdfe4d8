/* scene_accel.cpp - meshes, instances, BLAS builds and the TLAS slots of the render core (scene_accel.h).

   The acceleration structure is our own binned-SAH BVH2 (bvh_build.cpp) or GPU PLOC build (bvh_gpu.hip), collapsed to a
   BVH4, instead of the closed OptiX Prime BLAS/TLAS (core_mesh.cpp:53-66, rendercore.cpp:250-270). */
#include "scene_accel.h"

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>

#include "lh2_device.h"

namespace lh2 {

/* mat4::Inverted (RenderSystem/common_types.h:586-628); same formula as the oracle */
static void Mat4Inverse( const float* c, float* out )
{
	const float inv[16] = {
		c[5] * c[10] * c[15] - c[5] * c[11] * c[14] - c[9] * c[6] * c[15] + c[9] * c[7] * c[14] + c[13] * c[6] * c[11] - c[13] * c[7] * c[10],
		-c[1] * c[10] * c[15] + c[1] * c[11] * c[14] + c[9] * c[2] * c[15] - c[9] * c[3] * c[14] - c[13] * c[2] * c[11] + c[13] * c[3] * c[10],
		c[1] * c[6] * c[15] - c[1] * c[7] * c[14] - c[5] * c[2] * c[15] + c[5] * c[3] * c[14] + c[13] * c[2] * c[7] - c[13] * c[3] * c[6],
		-c[1] * c[6] * c[11] + c[1] * c[7] * c[10] + c[5] * c[2] * c[11] - c[5] * c[3] * c[10] - c[9] * c[2] * c[7] + c[9] * c[3] * c[6],
		-c[4] * c[10] * c[15] + c[4] * c[11] * c[14] + c[8] * c[6] * c[15] - c[8] * c[7] * c[14] - c[12] * c[6] * c[11] + c[12] * c[7] * c[10],
		c[0] * c[10] * c[15] - c[0] * c[11] * c[14] - c[8] * c[2] * c[15] + c[8] * c[3] * c[14] + c[12] * c[2] * c[11] - c[12] * c[3] * c[10],
		-c[0] * c[6] * c[15] + c[0] * c[7] * c[14] + c[4] * c[2] * c[15] - c[4] * c[3] * c[14] - c[12] * c[2] * c[7] + c[12] * c[3] * c[6],
		c[0] * c[6] * c[11] - c[0] * c[7] * c[10] - c[4] * c[2] * c[11] + c[4] * c[3] * c[10] + c[8] * c[2] * c[7] - c[8] * c[3] * c[6],
		c[4] * c[9] * c[15] - c[4] * c[11] * c[13] - c[8] * c[5] * c[15] + c[8] * c[7] * c[13] + c[12] * c[5] * c[11] - c[12] * c[7] * c[9],
		-c[0] * c[9] * c[15] + c[0] * c[11] * c[13] + c[8] * c[1] * c[15] - c[8] * c[3] * c[13] - c[12] * c[1] * c[11] + c[12] * c[3] * c[9],
		c[0] * c[5] * c[15] - c[0] * c[7] * c[13] - c[4] * c[1] * c[15] + c[4] * c[3] * c[13] + c[12] * c[1] * c[7] - c[12] * c[3] * c[5],
		-c[0] * c[5] * c[11] + c[0] * c[7] * c[9] + c[4] * c[1] * c[11] - c[4] * c[3] * c[9] - c[8] * c[1] * c[7] + c[8] * c[3] * c[5],
		-c[4] * c[9] * c[14] + c[4] * c[10] * c[13] + c[8] * c[5] * c[14] - c[8] * c[6] * c[13] - c[12] * c[5] * c[10] + c[12] * c[6] * c[9],
		c[0] * c[9] * c[14] - c[0] * c[10] * c[13] - c[8] * c[1] * c[14] + c[8] * c[2] * c[13] + c[12] * c[1] * c[10] - c[12] * c[2] * c[9],
		-c[0] * c[5] * c[14] + c[0] * c[6] * c[13] + c[4] * c[1] * c[14] - c[4] * c[2] * c[13] - c[12] * c[1] * c[6] + c[12] * c[2] * c[5],
		c[0] * c[5] * c[10] - c[0] * c[6] * c[9] - c[4] * c[1] * c[10] + c[4] * c[2] * c[9] + c[8] * c[1] * c[6] - c[8] * c[2] * c[5] };
	const float det = c[0] * inv[0] + c[1] * inv[4] + c[2] * inv[8] + c[3] * inv[12];
	if (det != 0) { const float invdet = 1.0f / det; for (int i = 0; i < 16; i++) out[i] = inv[i] * invdet; }
	else for (int i = 0; i < 16; i++) out[i] = (i % 5 == 0) ? 1.0f : 0.0f;
}

/* the box of a mesh box's eight corners under the instance matrix T */
static Aabb TransformBox( const float* T, const float* lo, const float* hi )
{
	Aabb b;
	for (int k = 0; k < 3; k++) b.lo[k] = 1e30f, b.hi[k] = -1e30f;
	for (int c = 0; c < 8; c++)
	{
		const float p[3] = { (c & 1) ? hi[0] : lo[0], (c & 2) ? hi[1] : lo[1], (c & 4) ? hi[2] : lo[2] };
		for (int k = 0; k < 3; k++)
		{
			const float* r = T + k * 4;
			const float v = r[0] * p[0] + r[1] * p[1] + r[2] * p[2] + r[3];
			b.lo[k] = std::min( b.lo[k], v ), b.hi[k] = std::max( b.hi[k], v );
		}
	}
	return b;
}

/* adds its lifetime to the host time the BLAS builds took (SceneAccel::BuildSeconds) */
struct BuildTimer
{
	float& total;
	const std::chrono::high_resolution_clock::time_point t0 = std::chrono::high_resolution_clock::now();
	~BuildTimer() { total += std::chrono::duration<float>( std::chrono::high_resolution_clock::now() - t0 ).count(); }
};

void SceneAccel::Init( hipStream_t core, hipStream_t ahead )
{
	stream = core, aheadStream = ahead;
	for (auto& e : evStage) CHK_HIP( hipEventCreateWithFlags( &e, hipEventDisableTiming ) );
	dSceneError.resize( 2 ), dTlasDepth.resize( 1 ), dBlasQError.resize( 1 );
	CHK_HIP( hipMemsetAsync( dSceneError.ptr, 0, sizeof( int ) * 2, stream ) );
	CHK_HIP( hipEventCreateWithFlags( &evTlasReady, hipEventDisableTiming ) );
	for (auto& e : evTlasFree) CHK_HIP( hipEventCreateWithFlags( &e, hipEventDisableTiming ) );
	CHK_HIP( hipMemsetAsync( dTlasDepth.ptr, 0, sizeof( int ), stream ) );
	CHK_HIP( hipMemsetAsync( dBlasQError.ptr, 0, sizeof( int ), stream ) );
	for (auto& d : dInstDesc)   /* shading reads record 0 for a miss (HitInstance): it always exists */
	{
		d.resize( 1 );
		CHK_HIP( hipMemsetAsync( d.ptr, 0, sizeof( lh2_CoreInstanceDesc ), stream ) );
	}
}

void SceneAccel::Shutdown()
{
	for (auto* m : meshes) delete m;
	meshes.clear();
	instances.clear();
	for (auto& e : evStage) (void)hipEventDestroy( e );
	for (hipEvent_t* e : { &evTlasReady, &evTlasFree[0], &evTlasFree[1] }) { if (*e) (void)hipEventDestroy( *e ); *e = nullptr; }
	for (int i = 0; i < 2; i++) { if (stage[i]) (void)hipHostFree( stage[i] ); stage[i] = nullptr, stageBytes[i] = 0; }
}

static std::atomic<int> gBlasBuilds{ 0 };
int SceneAccel::BlasBuildCount() { return gBlasBuilds.load(); }
void HostBlas::Run( int threads )
{
	std::call_once( once, [&] { job( *this, threads ); job = nullptr; gBlasBuilds++; } );
}

/* the mesh's slot (rendercore.cpp:215-223 + core_mesh.cpp:36-67: meshes arrive first-time in sequential order), with its
   shading triangles uploaded; the caller's triangle array is borrowed until the caller synchronizes the stream */
CoreMeshHost& SceneAccel::TakeMesh( int meshIdx, int triangleCount, const lh2_CoreTri* tris )
{
	if (meshIdx < 0 || meshIdx > (int)meshes.size()) FatalError( "SetGeometry: mesh index %d out of sequence", meshIdx );
	if (meshIdx == (int)meshes.size()) meshes.push_back( new CoreMeshHost() );
	CoreMeshHost& m = *meshes[meshIdx];
	m.triCount = triangleCount;
	m.shadeTris.upload( (const float4*)tris, (size_t)triangleCount * 11, stream );
	m.shadeTris.resize( 11 );
	return m;
}

void SceneAccel::SetGeometry( int meshIdx, int triangleCount, const lh2_CoreTri* tris )
{
	BuildTimer timer{ buildSeconds };
	CoreMeshHost& m = TakeMesh( meshIdx, triangleCount, tris );
	m.build = nullptr;   /* a build of earlier data not run yet is superseded */
	bool cpuBuild = !(gpuBuild && triangleCount >= 2);
	if (!cpuBuild)
	{
		/* GPU PLOC build straight from the uploaded CoreTri records (bvh_gpu.h) */
		float4 *nodes = nullptr, *tris48 = nullptr;
		GpuBuildResult r;
		SyncTlas();   /* a TLAS build queued on the ahead stream uses the same builder scratch: this build follows it */
		gpuBvh.BuildBlas( m.shadeTris.ptr, triangleCount, build.maxLeaf, 1.0f, &nodes, &tris48, r, stream );
		m.bvhNodes.adopt( nodes, (size_t)r.nodeCount * 4 );
		m.bvhTris.adopt( tris48, (size_t)triangleCount * 3 );
		m.leafTris = triangleCount;
		m.nodeCount = r.nodeCount, m.maxDepth = r.maxDepth;
		for (int k = 0; k < 3; k++) m.aabbLo[k] = r.lo[k], m.aabbHi[k] = r.hi[k];
		/* pathological inputs (e.g. long runs of nearly coincident triangles) can make a clustered tree
		   deep; the top-down SAH build bounds the depth by splitting such ranges in the middle */
		if (r.maxDepth > LH2_STACK_TOTAL / 2) cpuBuild = true;
	}
	if (cpuBuild)
	{
		/* CPU binned-SAH build (bvh_build.cpp), deferred: the inputs are copied now (the caller's triangle
		   array is borrowed for this call only) and the builds of all meshes set since the last one run in
		   parallel over the meshes when the scene is first needed (FlushBuilds) */
		std::vector<Aabb> prims( triangleCount );
		std::vector<float> verts( (size_t)triangleCount * 9 );
		for (int k = 0; k < 3; k++) m.aabbLo[k] = 1e30f, m.aabbHi[k] = -1e30f;
		for (int i = 0; i < triangleCount; i++)
		{
			const lh2_CoreTri& t = tris[i];
			const float v[9] = { t.vertex0.x, t.vertex0.y, t.vertex0.z, t.vertex1.x, t.vertex1.y, t.vertex1.z, t.vertex2.x, t.vertex2.y, t.vertex2.z };
			memcpy( &verts[(size_t)i * 9], v, sizeof( v ) );
			for (int k = 0; k < 3; k++)
			{
				prims[i].lo[k] = std::min( std::min( v[k], v[3 + k] ), v[6 + k] );
				prims[i].hi[k] = std::max( std::max( v[k], v[3 + k] ), v[6 + k] );
				m.aabbLo[k] = std::min( m.aabbLo[k], prims[i].lo[k] ), m.aabbHi[k] = std::max( m.aabbHi[k], prims[i].hi[k] );
			}
		}
		m.build = std::make_shared<HostBlas>();
		m.build->settings = build;
		m.build->job = [prims = std::move( prims ), verts = std::move( verts ), bs = build]( HostBlas& r, int threads ) {
			BvhOutput bvh;
			BuildBvh2( prims, bs.maxLeaf, threads, bvh, 1.0f, 0, bs.spatial > 0 ? verts.data() : nullptr, bs.spatial, bs.spatialBudget, bs.spatialMinRefs );
			/* one triangle record per leaf slot (a spatial split can reference a triangle from several leaves):
			   v0, e1 = v1 - v0, e2 = v2 - v0 in fp32, exactly as the oracle's intersect_tri */
			std::vector<float>& t48 = r.tris48;
			t48.assign( std::max<size_t>( bvh.perm.size(), 1 ) * 12, 0.0f );
			for (size_t j = 0; j < bvh.perm.size(); j++)
			{
				const uint32_t ti = bvh.perm[j];
				const float* v = &verts[(size_t)ti * 9];
				float* o = &t48[j * 12];
				o[0] = v[0], o[1] = v[1], o[2] = v[2]; memcpy( &o[3], &ti, 4 );
				o[4] = v[3] - v[0], o[5] = v[4] - v[1], o[6] = v[5] - v[2], o[7] = 0;
				o[8] = v[6] - v[0], o[9] = v[7] - v[1], o[10] = v[8] - v[2], o[11] = 0;
			}
			r.leafTris = (int)bvh.perm.size();
			r.nodeCount = (int)(bvh.nodes.size() / 16), r.maxDepth = bvh.maxDepth;
			r.nodes4.clear(), r.depth4 = 0;
			/* BVH4 collapse: dynamic programming (surface-area costs: node step 1, leaf visit 0.4, triangle test 0.5,
			   one triangle per leaf; merged leaves run the leaf loop divergent: slower, r02s) or greedy */
			if (bs.bvh4) r.depth4 = bs.bvh4Collapse ? CollapseBvh4Sah( bvh.nodes.data(), (size_t)r.nodeCount, r.nodes4, 0.4f, 0.5f, 1 )
				: CollapseBvh4( bvh.nodes.data(), (size_t)r.nodeCount, r.nodes4 );
			r.nodes2 = std::move( bvh.nodes );
		};
		pendingBuilds = true;
	}
	else if (build.bvh4)
	{
		/* GPU-built BLAS: collapse on the host (one download of the BVH2) */
		std::vector<float> n2( (size_t)m.nodeCount * 16 );
		CHK_HIP( hipMemcpyAsync( n2.data(), m.bvhNodes.ptr, n2.size() * sizeof( float ), hipMemcpyDeviceToHost, stream ) );
		CHK_HIP( hipStreamSynchronize( stream ) );
		BuildBlas4( m, n2.data() );
	}
	CHK_HIP( hipStreamSynchronize( stream ) );   /* the caller's triangle array is borrowed for this call only */
	geometryDirty = true;
}

/* the deferred CPU BLAS builds (SetGeometry), in parallel over the meshes on up to `buildThreads` host threads
   (a mesh's own build gets the threads left over when there are fewer meshes than threads), then their upload */
void SceneAccel::FlushBuilds()
{
	if (!pendingBuilds) return;
	pendingBuilds = false;
	BuildTimer timer{ buildSeconds };
	std::vector<CoreMeshHost*> jobs;
	for (auto* m : meshes) if (m->build) jobs.push_back( m );
	int workers = buildThreads;
	if (workers <= 0)
	{
		const char* e = getenv( "LH2_BUILD_THREADS" );
		if (!e) e = getenv( "OMP_NUM_THREADS" );
		const unsigned hw = std::thread::hardware_concurrency();
		workers = e && atoi( e ) > 0 ? atoi( e ) : (int)std::min( 16u, hw ? hw : 4u );
	}
	const int nthreads = std::max( 1, std::min( workers, (int)jobs.size() ) );
	const int perJob = std::max( 1, workers / std::max( 1, (int)jobs.size() ) );
	std::atomic<int> next{ 0 }, inUse{ 0 };
	std::vector<std::string> errors( nthreads );
	/* the last jobs, fewer than the workers, get the idle workers' share as threads of their own build (SBVH subtrees):
	   a job is granted threads only out of those no running build holds, so the total stays near `workers` */
	auto work = [&]( int w ) {
		try
		{
			for (int j; (j = next.fetch_add( 1 )) < (int)jobs.size();)
			{
				const int remaining = (int)jobs.size() - j;
				const int want = std::max( perJob, std::min( 8, workers / std::max( 1, remaining ) ) );
				/* reserve the grant atomically out of the threads no running build holds (one at least: this worker's own) */
				int held = inUse.load(), grant = 1;
				do grant = std::max( 1, std::min( want, workers - held ) );
				while (!inUse.compare_exchange_weak( held, held + grant ));
				jobs[j]->build->Run( grant );
				inUse -= grant;
			}
		}
		catch (const std::exception& e) { errors[w] = e.what(); }
	};
	std::vector<std::thread> pool;
	for (int w = 1; w < nthreads; w++) pool.emplace_back( work, w );
	work( 0 );
	for (auto& t : pool) t.join();
	for (auto& e : errors) if (!e.empty()) FatalError( "BLAS build: %s", e.c_str() );
	for (auto* m : jobs)
	{
		const HostBlas& r = *m->build;
		m->leafTris = r.leafTris, m->nodeCount = r.nodeCount, m->maxDepth = r.maxDepth, m->depth4 = r.depth4;
		m->bvhNodes.upload( (const float4*)r.nodes2.data(), r.nodes2.size() / 4, stream );
		m->bvhTris.upload( (const float4*)r.tris48.data(), r.tris48.size() / 4, stream );
		if (build.bvh4) m->bvh4Nodes.upload( (const float4*)r.nodes4.data(), r.nodes4.size() / 4, stream ), m->node4Count = (int)(r.nodes4.size() / 32);
		CHK_HIP( hipStreamSynchronize( stream ) );
		m->build.reset();   /* the last core to upload a shared build frees its host arrays */
	}
}

/* MultiDevice's sub-cores: the mesh of src (core 0, which has just taken it through SetGeometry), its shading triangles
   uploaded to this device, its deferred CPU build shared (run once by the first core to flush, uploaded by each).  A GPU
   build (gpuBuild), a mesh src has already uploaded, or a build made under other settings than this core's (HostBlas records
   them; MultiDevice::Setting keeps the sub-cores' settings equal, so the public API never gets there) is built here as
   SetGeometry builds it */
void SceneAccel::AdoptGeometry( int meshIdx, int triangleCount, const lh2_CoreTri* tris, const SceneAccel& src )
{
	const CoreMeshHost* sm = meshIdx >= 0 && meshIdx < (int)src.meshes.size() ? src.meshes[meshIdx] : nullptr;
	if (!sm || !sm->build || sm->triCount != triangleCount || !(sm->build->settings == build))
	{
		SetGeometry( meshIdx, triangleCount, tris );
		return;
	}
	BuildTimer timer{ buildSeconds };
	CoreMeshHost& m = TakeMesh( meshIdx, triangleCount, tris );
	for (int k = 0; k < 3; k++) m.aabbLo[k] = sm->aabbLo[k], m.aabbHi[k] = sm->aabbHi[k];
	m.build = sm->build;
	pendingBuilds = true;
	CHK_HIP( hipStreamSynchronize( stream ) );   /* the caller's triangle array is borrowed for this call only */
	geometryDirty = true;
}

void SceneAccel::BuildBlas4( CoreMeshHost& m, const float* nodes2 )
{
	std::vector<float> n4;
	/* bvh4Collapse 1: dynamic-programming collapse (surface-area costs, optional leaf merging); 0: greedy */
	/* node step = 1, leaf visit 0.4, triangle test 0.5; one triangle per leaf (merged leaves run the leaf loop
	   divergent: slower, profiles/r02s_ab_collapse_shade4.txt) */
	m.depth4 = build.bvh4Collapse ? CollapseBvh4Sah( nodes2, (size_t)m.nodeCount, n4, 0.4f, 0.5f, 1 )
		: CollapseBvh4( nodes2, (size_t)m.nodeCount, n4 );
	m.bvh4Nodes.upload( (const float4*)n4.data(), n4.size() / 4, stream );
	m.node4Count = (int)(n4.size() / 32);
}

void SceneAccel::SetInstance( int instanceIdx, int meshIdx, const float* M )   /* rendercore.cpp:229-243 */
{
	/* host state only: UpdateToplevel writes it into the TLAS slot no frame in flight reads */
	if (meshIdx == -1) { if ((int)instances.size() > instanceIdx) instances.resize( instanceIdx ); instancesDirty = true; return; }
	if (meshIdx < 0 || meshIdx >= (int)meshes.size()) FatalError( "SetInstance: unknown mesh %d", meshIdx );
	if (instanceIdx >= (int)instances.size()) instances.resize( instanceIdx + 1 );
	instances[instanceIdx].mesh = meshIdx;
	memcpy( instances[instanceIdx].T, M, 64 );
	instancesDirty = true;
}

/* scene node array = all BLAS (relocated, device to device) followed by room for the TLAS */
void SceneAccel::ConcatenateBlas( int ni )
{
	FlushBuilds();
	meshNodeBase.assign( meshes.size(), 0 ), meshTriBase.assign( meshes.size(), 0 ), meshNode4Base.assign( meshes.size(), 0 );
	int nodeTotal = 0, triTotal = 0, node4Total = 0, meshTris = 0;
	maxBlasDepth = 0, maxBlas4Depth = 0;
	std::vector<float> bounds( std::max<size_t>( meshes.size(), 1 ) * 6, 0.0f );
	for (size_t mi = 0; mi < meshes.size(); mi++)
	{
		const CoreMeshHost& m = *meshes[mi];
		meshNodeBase[mi] = nodeTotal, meshTriBase[mi] = triTotal, meshNode4Base[mi] = node4Total;
		nodeTotal += m.nodeCount, triTotal += m.leafTris, node4Total += m.node4Count, meshTris += m.triCount;
		maxBlasDepth = std::max( maxBlasDepth, m.maxDepth ), maxBlas4Depth = std::max( maxBlas4Depth, m.depth4 );
		for (int k = 0; k < 3; k++) bounds[mi * 6 + k] = m.aabbLo[k], bounds[mi * 6 + 3 + k] = m.aabbHi[k];
		if (m.triCount == 0) bounds[mi * 6] = 1.0f, bounds[mi * 6 + 3] = 0.0f;   /* empty-mesh marker */
	}
	tlasCapacity = std::max( 64, 2 * ni + 16 );
	/* frames in flight may still read the old arrays, and a TLAS update may be queued on the ahead stream */
	CHK_HIP( hipStreamSynchronize( stream ) );
	CHK_HIP( hipStreamSynchronize( aheadStream ) );
	dNodes.free(), dTris.free(), dNodes4.free(), dNodes4q.free();
	/* after the BLAS: two TLAS slots of tlasCapacity nodes each (UpdateToplevel) */
	dNodes.resize( ((size_t)nodeTotal + 2 * tlasCapacity) * 4 );
	/* the BVH4 loops address nodes with 32-bit buffer offsets (lh2_trace4d.inc): the array stays below 2 GiB */
	if (build.bvh4 && ((size_t)node4Total + 2 * tlasCapacity) * 128 > 0x7fffffffull)
		FatalError( "BVH4 of %zu nodes exceeds the 2 GiB the traversal addresses", (size_t)node4Total + 2 * tlasCapacity );
	if (build.bvh4) dNodes4.resize( ((size_t)node4Total + 2 * tlasCapacity) * 8 ), dNodes4q.resize( ((size_t)node4Total + 2 * tlasCapacity) * 4 );
	dTris.resize( (size_t)std::max( triTotal, 1 ) * 3 );
	/* the TLAS region starts as NaN boxes: a TLAS of fewer nodes than the capacity leaves no uninitialised (possibly huge,
	   finite) boxes behind it for the quantizer's range check (k_quantize4) */
	CHK_HIP( hipMemsetAsync( dNodes.ptr + (size_t)nodeTotal * 4, 0xff, sizeof( float4 ) * 4 * 2 * (size_t)tlasCapacity, stream ) );
	dBlasQError.resize( 1 );
	CHK_HIP( hipMemsetAsync( dBlasQError.ptr, 0, sizeof( int ), stream ) );
	for (size_t mi = 0; mi < meshes.size(); mi++)
	{
		const CoreMeshHost& m = *meshes[mi];
		GpuBvhBuilder::Relocate( m.bvhNodes.ptr, m.nodeCount, meshNodeBase[mi], (uint32_t)meshTriBase[mi], dNodes.ptr, stream );
		if (build.bvh4) GpuBvhBuilder::Relocate4( m.bvh4Nodes.ptr, m.node4Count, meshNode4Base[mi], (uint32_t)meshTriBase[mi], dNodes4.ptr, stream );
		if (m.leafTris) CHK_HIP( hipMemcpyAsync( dTris.ptr + (size_t)meshTriBase[mi] * 3, m.bvhTris.ptr, sizeof( float4 ) * 3 * (size_t)m.leafTris, hipMemcpyDeviceToDevice, stream ) );
	}
	if (build.bvh4) GpuBvhBuilder::Quantize4( dNodes4.ptr, 0, node4Total, dNodes4q.ptr, dBlasQError.ptr, stream );
	dMeshBounds.upload( bounds.data(), bounds.size(), stream );
	CHK_HIP( hipStreamSynchronize( stream ) );
	blasNodeCount = nodeTotal, blasTriCount = triTotal, blasNode4Count = node4Total, blasMeshTris = meshTris;
	geometryDirty = false;
}

bool SceneAccel::UpdateToplevel()   /* rendercore.cpp:250-270 (TLAS) + :481-505 (instance descriptors) */
{
	const int ni = (int)instances.size();
	const bool relaid = geometryDirty || ni + 1 > tlasCapacity;
	if (relaid) ConcatenateBlas( ni );
	/* the TLAS slot no frame in flight reads (the other one is the last frame's), written on the ahead stream behind the
	   last frame that read it; instance-only updates are no new scene data to the caller, so the next frame may still overlap */
	const int ts = tlasSlot ^ 1;
	hipStream_t us = aheadStream;
	if (tlasFreeValid[ts]) CHK_HIP( hipStreamWaitEvent( us, evTlasFree[ts], 0 ) );
	tlasRoot = TlasBase2( ts );
	/* host part: inverse transforms and instance records, written to pinned staging (double-buffered)
	   and copied asynchronously; no host-device round trip per frame */
	const int slot = stageSlot;
	stageSlot ^= 1;
	const size_t nRec = (size_t)std::max( ni, 1 );
	const size_t offInst = 0, offDesc = offInst + nRec * sizeof( DevInstance ), offT = offDesc + nRec * sizeof( lh2_CoreInstanceDesc );
	const size_t offMesh = offT + nRec * 64, offNodes = offMesh + nRec * 4, need = offNodes + 4 * 64 * nRec + 64;
	CHK_HIP( hipEventSynchronize( evStage[slot] ) );   /* the copies from this slot two updates ago are done */
	if (need > stageBytes[slot])
	{
		if (stage[slot]) CHK_HIP( hipHostFree( stage[slot] ) );
		stageBytes[slot] = need + need / 2;
		CHK_HIP( hipHostMalloc( (void**)&stage[slot], stageBytes[slot], hipHostMallocDefault ) );
	}
	uint8_t* sb = stage[slot];
	DevInstance* di = (DevInstance*)(sb + offInst);
	lh2_CoreInstanceDesc* desc = (lh2_CoreInstanceDesc*)(sb + offDesc);
	float* Ts = (float*)(sb + offT);
	int* meshIds = (int*)(sb + offMesh);
	memset( sb, 0, offMesh + nRec * 4 );
	for (int i = 0; i < ni; i++)
	{
		CoreInstanceHost& in = instances[i];
		Mat4Inverse( in.T, in.inv );
		di[i].inv0 = make_float4( in.inv[0], in.inv[1], in.inv[2], in.inv[3] );
		di[i].inv1 = make_float4( in.inv[4], in.inv[5], in.inv[6], in.inv[7] );
		di[i].inv2 = make_float4( in.inv[8], in.inv[9], in.inv[10], in.inv[11] );
		di[i].root = meshNodeBase[in.mesh], di[i].triBase = meshTriBase[in.mesh], di[i].mesh = in.mesh;
		di[i].root4 = build.bvh4 ? meshNode4Base[in.mesh] : 0;
		desc[i].triangles = meshes[in.mesh]->shadeTris.ptr;
		desc[i].A = { in.inv[0], in.inv[1], in.inv[2], in.inv[3] };
		desc[i].B = { in.inv[4], in.inv[5], in.inv[6], in.inv[7] };
		desc[i].C = { in.inv[8], in.inv[9], in.inv[10], in.inv[11] };
		desc[i].D = { in.inv[12], in.inv[13], in.inv[14], in.inv[15] };
		memcpy( Ts + (size_t)i * 16, in.T, 64 );
		meshIds[i] = in.mesh;
	}
	/* the scene's world box (instance transforms of the mesh boxes): the shade launches order extension
	   rays by their chord through it (ShadeParams::chordCut) */
	for (int k = 0; k < 3; k++) sceneLo[k] = 1e30f, sceneHi[k] = -1e30f;
	for (int i = 0; i < ni; i++)
	{
		const CoreInstanceHost& in = instances[i];
		const CoreMeshHost& m = *meshes[in.mesh];
		if (m.triCount == 0) continue;
		const Aabb b = TransformBox( in.T, m.aabbLo, m.aabbHi );
		for (int k = 0; k < 3; k++) sceneLo[k] = std::min( sceneLo[k], b.lo[k] ), sceneHi[k] = std::max( sceneHi[k], b.hi[k] );
	}
	/* the quantized nodes' origins lie in these boxes (TLAS: world; BLAS: mesh space); 1 % slack for the
	   device-side TLAS bounds' own rounding */
	qBound = 0;
	for (int k = 0; k < 3; k++) qBound = std::max( qBound, std::max( fabsf( sceneLo[k] ), fabsf( sceneHi[k] ) ) );
	for (const auto& m : meshes)
		if (m->triCount) for (int k = 0; k < 3; k++) qBound = std::max( qBound, std::max( fabsf( m->aabbLo[k] ), fabsf( m->aabbHi[k] ) ) );
	qBound = qBound * 1.01f + 1e-30f;
	/* a slot's tables grow only with the work that may read them drained (DevBuf::resize frees the old buffer) */
	if (dInst[ts].count < nRec * sizeof( DevInstance ) || dInstDesc[ts].count < nRec || dInstT.count < nRec * 16 || dInstMesh.count < nRec)
	{
		CHK_HIP( hipStreamSynchronize( stream ) );
		CHK_HIP( hipStreamSynchronize( us ) );
		dInst[ts].resize( nRec * sizeof( DevInstance ) ), dInstDesc[ts].resize( nRec ), dInstT.resize( nRec * 16 ), dInstMesh.resize( nRec );
	}
	CHK_HIP( hipMemcpyAsync( dInst[ts].ptr, di, nRec * sizeof( DevInstance ), hipMemcpyHostToDevice, us ) );
	CHK_HIP( hipMemcpyAsync( dInstDesc[ts].ptr, desc, nRec * sizeof( lh2_CoreInstanceDesc ), hipMemcpyHostToDevice, us ) );
	/* the scene error starts as the BLAS quantizer's (ConcatenateBlas), the TLAS checks add to it */
	CHK_HIP( hipMemcpyAsync( SceneErr( ts ), dBlasQError.ptr, sizeof( int ), hipMemcpyDeviceToDevice, us ) );
	int tlasNodes = 1;   /* the nodes this TLAS has (the slot holds tlasCapacity): the BVH4 copy and the quantizer touch no others */
	if (ni >= 2 && gpuTlas)
	{
		/* TLAS built on the device from the instance transforms (bvh_gpu.h) */
		CHK_HIP( hipMemcpyAsync( dInstT.ptr, Ts, nRec * 64, hipMemcpyHostToDevice, us ) );
		CHK_HIP( hipMemcpyAsync( dInstMesh.ptr, meshIds, nRec * 4, hipMemcpyHostToDevice, us ) );
		GpuTlasArgs ta;
		ta.T = dInstT.ptr, ta.instMesh = dInstMesh.ptr, ta.meshBounds = dMeshBounds.ptr, ta.count = ni;
		ta.nodeBase = TlasBase2( ts ), ta.nodes = dNodes.ptr, ta.maxBlasDepth = StackDepthBound();
		ta.sceneError = SceneErr( ts ), ta.tlasDepth = dTlasDepth.ptr;
		ta.tlasFactor = 1;
		gpuBvh.BuildTlas( ta, us );
		tlasNodes = ni - 1;   /* one instance per leaf: ni - 1 child-pair nodes, dense in preorder (bvh_gpu.hip emit_node) */
		tlasOnDevice = true;
		sceneMaxDepth = -1;   /* known on the device; SceneInfo reads it */
	}
	else
	{
		/* host TLAS (binned SAH) over instance world bounds, 1 instance per leaf */
		std::vector<Aabb> prims;
		std::vector<int> primInst;
		for (int i = 0; i < ni; i++)
		{
			const CoreInstanceHost& in = instances[i];
			const CoreMeshHost& m = *meshes[in.mesh];
			if (m.triCount == 0) continue;
			Aabb b = TransformBox( in.T, m.aabbLo, m.aabbHi );
			/* pad by a relative epsilon: the ray is transformed in fp32 on the device */
			for (int k = 0; k < 3; k++)
			{
				const float e = 1e-5f * std::max( std::fabs( b.lo[k] ), std::fabs( b.hi[k] ) ) + 1e-30f;
				b.lo[k] -= e, b.hi[k] += e;
			}
			prims.push_back( b ), primInst.push_back( i );
		}
		BvhOutput tlas;
		BuildBvh2( prims, 1, 1, tlas );
		const size_t tn = tlas.nodes.size() / 16;
		if (tn > (size_t)tlasCapacity) FatalError( "TLAS of %zu nodes exceeds its capacity %d", tn, tlasCapacity );
		tlasNodes = std::max( 1, (int)tn );
		for (size_t k = 0; k < tn; k++)
		{
			int* refs = (int*)&tlas.nodes[k * 16 + 12];
			for (int c = 0; c < 2; c++)
			{
				if (refs[c] >= 0) refs[c] += TlasBase2( ts );
				else if (!prims.empty())
				{
					if (LEAF_COUNT( refs[c] ) != 1) FatalError( "TLAS leaf with %d instances", LEAF_COUNT( refs[c] ) );
					refs[c] = MAKE_LEAF( (uint32_t)primInst[tlas.perm[LEAF_FIRST( refs[c] )]], 1 );
				}
			}
		}
		if (tlas.nodes.size() * sizeof( float ) > need - offNodes) FatalError( "TLAS staging overflow" );
		memcpy( sb + offNodes, tlas.nodes.data(), tlas.nodes.size() * sizeof( float ) );
		CHK_HIP( hipMemcpyAsync( dNodes.ptr + (size_t)TlasBase2( ts ) * 4, sb + offNodes, tlas.nodes.size() * sizeof( float ), hipMemcpyHostToDevice, us ) );
		sceneMaxDepth = tlas.maxDepth + StackDepthBound();
		tlasOnDevice = false;
		if (sceneMaxDepth >= LH2_STACK_TOTAL - 1) FatalError( "BVH depth %d exceeds the traversal stack (%d)", sceneMaxDepth, LH2_STACK_TOTAL );
	}
	/* the TLAS in the BVH4 array: its BVH2 nodes as two-child BVH4 nodes (one short launch), quantized.  Only the nodes this
	   TLAS has: the slot's nodes beyond them hold an earlier, larger TLAS or memory never written, whose boxes (possibly huge,
	   finite) would set the quantizer's range error (round 4 fixed that by NaN-filling the region, 651cce0; no traversal ever
	   reaches such a node, so it is not read at all now; test_gpu_parity.py::test_stale_tlas_region_is_not_quantized) */
	if (build.bvh4)
	{
		GpuBvhBuilder::TlasToBvh4( dNodes.ptr, TlasBase2( ts ), tlasNodes, TlasBase4( ts ), dNodes4.ptr, us );
		GpuBvhBuilder::Quantize4( dNodes4.ptr, TlasBase4( ts ), tlasNodes, dNodes4q.ptr, SceneErr( ts ), us );
	}
	tlasNodeCount[ts] = tlasNodes;
	CHK_HIP( hipEventRecord( evStage[slot], us ) );
	CHK_HIP( hipEventRecord( evTlasReady, us ) );
	tlasSlot = ts, tlasPending = true;
	instancesDirty = false;
	return relaid;
}

void SceneAccel::SyncTlas()
{
	if (!tlasPending) return;
	CHK_HIP( hipStreamWaitEvent( stream, evTlasReady, 0 ) );
	tlasPending = false;
}

void SceneAccel::ReleaseSlot( int s, hipStream_t st )
{
	CHK_HIP( hipEventRecord( evTlasFree[s], st ) );
	tlasFreeValid[s] = true;
}

void SceneAccel::Fill( SceneDev& s, bool singleInstanceStart )
{
	SyncTlas();
	s.nodes = dNodes.ptr, s.tris = dTris.ptr, s.inst = (const DevInstance*)dInst[tlasSlot].ptr;
	s.sceneError = SceneErr( tlasSlot );
	s.tlasRoot = tlasRoot, s.instCount = (int)instances.size();
	s.nodes4 = dNodes4.ptr, s.nodes4q = dNodes4q.ptr, s.qBound = qBound, s.tlasRoot4 = TlasBase4( tlasSlot );
	/* one instance of a non-empty mesh: rays start at its TLAS leaf (MAKE_LEAF( 0, 1 ) = ~0) and skip
	   the TLAS root's box test, which can only cull (TopLevelBVH::Traverse bvh.cpp:594-649); the
	   instance transform runs as at the leaf, so the hits are unchanged: one loop iteration less per ray */
	s.root40 = 0, s.tris0 = nullptr;
	if (singleInstanceStart && instances.size() == 1 && instances[0].mesh >= 0 && instances[0].mesh < (int)meshes.size() &&
		meshes[instances[0].mesh]->triCount > 0)
	{
		s.tlasRoot = s.tlasRoot4 = ~0;
		s.root40 = build.bvh4 ? meshNode4Base[instances[0].mesh] : 0;   /* DevInstance::root4 of instance 0 (UpdateToplevel) */
		s.tris0 = meshes[instances[0].mesh]->shadeTris.ptr;             /* lh2_CoreInstanceDesc::triangles of instance 0 */
	}
	s.instDesc = dInstDesc[tlasSlot].ptr;
}

void SceneAccel::SceneInfo( int* nodeCount, int* triCount, int* maxDepth, int* instCount )
{
	if (nodeCount) *nodeCount = blasNodeCount;
	if (triCount) *triCount = blasMeshTris;
	if (tlasOnDevice)
	{
		int d = 0;
		SyncTlas();
		CHK_HIP( hipMemcpyAsync( &d, dTlasDepth.ptr, sizeof( int ), hipMemcpyDeviceToHost, stream ) );
		CHK_HIP( hipStreamSynchronize( stream ) );
		sceneMaxDepth = d + maxBlasDepth;
	}
	if (maxDepth) *maxDepth = sceneMaxDepth;
	if (instCount) *instCount = (int)instances.size();
}

int SceneAccel::DebugBvh4( float* f32Nodes, uint32_t* qNodes, int cap )
{
	SyncTlas();
	CHK_HIP( hipStreamSynchronize( stream ) );
	if (!dNodes4.ptr || !dNodes4q.ptr) return 0;
	const int tn = tlasNodeCount[tlasSlot];   /* the current TLAS's own nodes (the slot's others are never written, §3) */
	if (cap <= 0 || !f32Nodes || !qNodes) return blasNode4Count + tn;   /* a count-only call */
	/* the BLAS nodes, then the current TLAS slot's */
	const int n = std::min( cap, blasNode4Count + tn ), nb = std::min( n, blasNode4Count ), nt = n - nb;
	CHK_HIP( hipMemcpy( f32Nodes, dNodes4.ptr, 128 * (size_t)nb, hipMemcpyDeviceToHost ) );
	CHK_HIP( hipMemcpy( qNodes, dNodes4q.ptr, 64 * (size_t)nb, hipMemcpyDeviceToHost ) );
	if (nt > 0)
	{
		CHK_HIP( hipMemcpy( f32Nodes + 32 * (size_t)nb, dNodes4.ptr + 8 * (size_t)TlasBase4( tlasSlot ), 128 * (size_t)nt, hipMemcpyDeviceToHost ) );
		CHK_HIP( hipMemcpy( qNodes + 16 * (size_t)nb, dNodes4q.ptr + 4 * (size_t)TlasBase4( tlasSlot ), 64 * (size_t)nt, hipMemcpyDeviceToHost ) );
	}
	return n;
}

/* diagnostics (test hook): fill both TLAS slots' node regions (BVH2 and BVH4, f32 and quantized) with `value`, as memory an
   earlier, larger TLAS or an uninitialised allocation leaves behind the nodes a TLAS update writes */
void SceneAccel::DebugPoisonTlas( float value )
{
	SyncTlas();
	CHK_HIP( hipStreamSynchronize( stream ) );
	CHK_HIP( hipStreamSynchronize( aheadStream ) );
	std::vector<float> fill( (size_t)2 * tlasCapacity * 32, value );
	CHK_HIP( hipMemcpy( dNodes.ptr + (size_t)blasNodeCount * 4, fill.data(), sizeof( float4 ) * 4 * 2 * (size_t)tlasCapacity, hipMemcpyHostToDevice ) );
	if (build.bvh4)
	{
		CHK_HIP( hipMemcpy( dNodes4.ptr + (size_t)blasNode4Count * 8, fill.data(), sizeof( float4 ) * 8 * 2 * (size_t)tlasCapacity, hipMemcpyHostToDevice ) );
		CHK_HIP( hipMemcpy( dNodes4q.ptr + (size_t)blasNode4Count * 4, fill.data(), sizeof( uint4 ) * 4 * 2 * (size_t)tlasCapacity, hipMemcpyHostToDevice ) );
	}
}

}  // namespace lh2
