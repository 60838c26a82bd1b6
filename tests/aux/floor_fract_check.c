/* Exhaustive check behind level_cell_in_cube (csrc/nerf_device.h): for every fp32 f in [0, 4096]
 *   - truncation to an unsigned integer (v_cvt_u32_f32) equals (uint32_t)(int)floorf(f), what level_cell computes, and
 *   - the exact fractional part of f (what v_fract_f32 returns for f >= 0; modff here) has the bits of the ROUNDED fp32
 *     subtraction f - floorf(f), i.e. that subtraction is exact and never reaches 1.
 * 4096 is above the largest fma(scale, x, 0.5) of any level the render kernels take through that path.
 * usage: floor_fract_check <stride>   -- prints the number of mismatches. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static inline uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

int main(int argc, char** argv) {
	uint32_t stride = argc > 1 ? (uint32_t)atoi(argv[1]) : 1u;
	if (stride == 0u) stride = 1u;
	const uint32_t hi = bits(4096.0f);
	long long bad = 0, n = 0;
#pragma omp parallel for reduction(+ : bad, n) schedule(static)
	for (uint32_t u = 0; u <= hi; u += stride) {
		const float f = from_bits(u);
		volatile float fl = floorf(f);
		volatile float sub = f - fl; /* level_cell: rounded to fp32 */
		float ip;
		const float fr = modff(f, &ip);
		if ((uint32_t)f != (uint32_t)(int)fl) ++bad;
		if (bits(fr) != bits(sub)) ++bad;
		if (!(fr < 1.0f)) ++bad;
		++n;
	}
	/* the range's end is part of it whatever the stride */
	{
		const float f = 4096.0f;
		float ip;
		if ((uint32_t)f != (uint32_t)(int)floorf(f) || bits(modff(f, &ip)) != bits(f - floorf(f))) ++bad;
	}
	fprintf(stderr, "%lld values\n", n);
	printf("%lld\n", bad);
	return bad != 0;
}
