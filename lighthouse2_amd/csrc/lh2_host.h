/* lh2_host.h - what every host file of the core shares: the error exit, the HIP call check and the device buffer */
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace lh2 {

void FatalError( const char* fmt, ... );

#define CHK_HIP( stmt ) do { hipError_t e_ = (stmt); if (e_ != hipSuccess) FatalError( "%s failed: %s (%s:%d)", #stmt, hipGetErrorString( e_ ), __FILE__, __LINE__ ); } while (0)

template <class T> struct DevBuf
{
	T* ptr = nullptr;
	size_t count = 0;
	DevBuf() = default;
	DevBuf( const DevBuf& ) = delete;
	DevBuf& operator=( const DevBuf& ) = delete;
	~DevBuf() { free(); }
	void free() { if (ptr) (void)hipFree( ptr ); ptr = nullptr; count = 0; }
	void resize( size_t n )   /* discards contents */
	{
		if (n <= count && ptr) return;
		free();
		if (n == 0) n = 1;
		if (hipMalloc( (void**)&ptr, n * sizeof( T ) ) != hipSuccess) FatalError( "hipMalloc of %zu bytes failed", n * sizeof( T ) );
		count = n;
	}
	void adopt( T* p, size_t n ) { free(); ptr = p, count = n; }   /* takes ownership of a hipMalloc'ed block */
	void upload( const T* src, size_t n, hipStream_t st )
	{
		resize( n );
		if (n) if (hipMemcpyAsync( ptr, src, n * sizeof( T ), hipMemcpyHostToDevice, st ) != hipSuccess) FatalError( "upload failed" );
	}
};

}  // namespace lh2
