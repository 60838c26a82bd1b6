// The nine real spherical harmonics of degree <= 2 and the clamped-cosine convolution of an SH9 irradiance probe (contract:
// include/ngp_hip.h, "SH9 irradiance volumes"). Plain C++ so that the lookup kernel (float) and ngp_irradiance_sh_eval on the host (double)
// evaluate one definition. Order, signs and constants are those of sh4_all's first nine outputs (nerf_device.h).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NGP_SH_FN __host__ __device__ __forceinline__
#else
#define NGP_SH_FN inline
#endif

namespace ngp {

constexpr uint32_t SH9_RECORD_FLOATS = 28; // c[3 m + ch], m = 0..8, ch = r, g, b; float 27 = w, the fraction of the probe's rays no mesh blocks

// Y_m of a unit direction
template <typename T>
NGP_SH_FN void sh9_basis(T x, T y, T z, T* Y) {
	Y[0] = (T)0.28209479177387814;
	Y[1] = (T)-0.48860251190291987 * y;
	Y[2] = (T)0.48860251190291987 * z;
	Y[3] = (T)-0.48860251190291987 * x;
	Y[4] = (T)1.0925484305920792 * (x * y);
	Y[5] = (T)-1.0925484305920792 * (y * z);
	Y[6] = (T)0.94617469575755997 * (z * z) - (T)0.31539156525251999;
	Y[7] = (T)-1.0925484305920792 * (x * z);
	Y[8] = (T)0.54627421529603959 * (x * x) - (T)0.54627421529603959 * (y * y);
}

// A_m: the clamped cosine's zonal coefficients times sqrt(4 pi / (2 l + 1)) (Ramamoorthi & Hanrahan 2001): pi, 2 pi / 3, pi / 4
template <typename T>
NGP_SH_FN T sh9_band_factor(int m) {
	return m == 0 ? (T)3.14159265358979323846 : m < 4 ? (T)2.09439510239319549231 : (T)0.78539816339744830962;
}

// E_ch = sum_m A_m c[3 m + ch] Y_m(n), n a unit vector; summed in the order m = 0..8. No clamp: the result can ring slightly negative.
template <typename T, typename C>
NGP_SH_FN void sh9_irradiance(const C* c, T x, T y, T z, T* E) {
	T Y[9];
	sh9_basis(x, y, z, Y);
	E[0] = E[1] = E[2] = (T)0;
#pragma unroll
	for (int m = 0; m < 9; ++m) {
		const T a = sh9_band_factor<T>(m) * Y[m];
		E[0] += a * (T)c[3 * m];
		E[1] += a * (T)c[3 * m + 1];
		E[2] += a * (T)c[3 * m + 2];
	}
}

} // namespace ngp
