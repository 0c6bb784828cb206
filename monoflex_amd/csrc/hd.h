// MFX_HD: a function of the *_math.h headers, compiled for host and device by hipcc and for the host alone by tests/shim.
#pragma once
#ifdef __HIPCC__
#define MFX_HD __host__ __device__ inline
#else
#define MFX_HD inline
#endif
