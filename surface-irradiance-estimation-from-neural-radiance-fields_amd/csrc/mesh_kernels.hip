// Geometry mode, mesh side, for MI355X (gfx950): one fused kernel per frame does what the reference spreads over
//   init_rays_with_payload_kernel_mesh_geometry -> mesh_raytrace_kernel -> prepare_shadow_rays_geometry ->
//   mesh_raytrace_kernel -> write_shadow_ray_result_geometry -> shade_kernel_mesh_geometry
// (src/testbed_geometry_training.cu:2202-2320, src/geometry_bvh.cu:646-676) with seven ray-state arrays in DRAM.
// Primary hit, sun shadow ray and BRDF stay in registers; the only traffic is BVH nodes / triangles (cache resident)
// and one frame/depth write per pixel. Software BVH4 traversal replaces OptiX (north_star: no OptiX).
#include "render_common.h"
#include "sh9.h"

#include <type_traits>

namespace ngp {

constexpr float MAX_DIST = 100.0f; // geometry_bvh.cu:23

NGP_DEV f3 ld3(const float* p) { return mk3(p[0], p[1], p[2]); }
NGP_DEV f3 cross3(f3 a, f3 b) { return mk3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
NGP_DEV bool box_contains(const float* bmin, const float* bmax, f3 p) {
	return p.x >= bmin[0] && p.x <= bmax[0] && p.y >= bmin[1] && p.y <= bmax[1] && p.z >= bmin[2] && p.z <= bmax[2];
}

// Triangle::ray_intersect, triangle.cuh:44-58
NGP_DEV float tri_ray_intersect(const Triangle& tri, f3 ro, f3 rd) {
	f3 a = ld3(tri.a);
	f3 v1v0 = sub3(ld3(tri.b), a);
	f3 v2v0 = sub3(ld3(tri.c), a);
	f3 rov0 = sub3(ro, a);
	f3 n = cross3(v1v0, v2v0);
	f3 q = cross3(rov0, rd);
	float d = 1.0f / dot3(rd, n);
	float u = d * -dot3(q, v2v0);
	float v = d * dot3(q, v1v0);
	float t = d * -dot3(n, rov0);
	if (u < 0.0f || u > 1.0f || v < 0.0f || (u + v) > 1.0f || t < 0.0f) t = 3.402823466e+38f;
	return t;
}

struct DistIdx {
	float dist;
	uint32_t idx;
};
NGP_DEV void cas(DistIdx& a, DistIdx& b) { // compare_and_swap with "<": sorts descending, triangle_bvh.cuh:161-176
	if (a.dist < b.dist) {
		DistIdx t = a;
		a = b;
		b = t;
	}
}

// GeometryBvh4::ray_intersect_triangle (geometry_bvh.cu:61-109) == TriangleBvh4::ray_intersect (triangle_bvh.cu:150-193)
NGP_DEV void bvh4_ray_intersect(const TriangleBvhNode* __restrict__ nodes, const Triangle* __restrict__ tris, f3 ro, f3 rd, int& out_idx, float& out_t) {
	int stack[BVH4_STACK_SIZE]; // deep enough for every BVH the builder lets through (ngp_kernels.h)
	int sp = 0;
	stack[sp++] = 0;
	float mint = MAX_DIST;
	int shortest = -1;
	while (sp > 0) {
		int idx = stack[--sp];
		const int left = nodes[idx].left_idx, right = nodes[idx].right_idx;
		if (left < 0) {
			int end = -right - 1;
			for (int i = -left - 1; i < end; ++i) {
				float t = tri_ray_intersect(tris[i], ro, rd);
				if (t < mint) {
					mint = t;
					shortest = i;
				}
			}
		} else {
			DistIdx ch[4];
#pragma unroll
			for (uint32_t i = 0; i < 4; ++i) {
				const TriangleBvhNode& c = nodes[left + (int)i];
				ch[i].dist = aabb_ray_entry(c.bmin, c.bmax, ro, rd);
				ch[i].idx = (uint32_t)left + i;
			}
			cas(ch[0], ch[2]); cas(ch[1], ch[3]); cas(ch[0], ch[1]); cas(ch[2], ch[3]); cas(ch[1], ch[2]);
#pragma unroll
			for (uint32_t i = 0; i < 4; ++i) {
				if (ch[i].dist < mint && sp < BVH4_STACK_SIZE) stack[sp++] = (int)ch[i].idx;
			}
		}
	}
	out_idx = shortest;
	out_t = mint;
}

// mesh_raytrace_kernel body (geometry_bvh.cu:646-676) + GeometryBvh4::ray_intersect leaf scan (:166-200)
// Kept as the reference has them (contract: ngp_trace_mesh_rays in include/ngp_hip.h):
//  - only the mesh whose box has the smallest slab entry below MAX_DIST is traced. The entry's sign is not looked at, so a box
//    behind the origin (a negative entry) beats every box ahead: a shadow ray, which starts on its own mesh, only ever sees that mesh;
//  - a ray whose line enters no box within MAX_DIST is left untouched. render_mesh_fused then finds its position, the camera's,
//    inside the scene box and shades the pixel with alpha 1, depth 0 and N = the ray's direction (NdotV = -1: the ambient term alone);
//  - a traced ray that hits nothing ends at pos + MAX_DIST * dir, its direction unchanged.
// hit: the traversal found a triangle (idx > -1). A ray that chose no mesh, or hit nothing in the one it chose, has none.
// WITH_ID (the material instantiations): *mesh_id receives the chosen mesh where the ray hit, else -1; without it mesh_id is not looked at.
template <bool WITH_ID = false>
NGP_DEV void trace_mesh(const MeshSceneParams& S, f3& pos, f3& dir, bool& hit, int* mesh_id = nullptr) {
	hit = false;
	if constexpr (WITH_ID) *mesh_id = -1;
	float mint = MAX_DIST;
	int mesh_idx = -1;
	for (uint32_t m = 0; m < S.n_meshes; ++m) {
		float t = aabb_ray_entry(S.meshes[m].bmin, S.meshes[m].bmax, pos, dir);
		if (t < mint && t > -3.402823466e+38f) {
			mint = t;
			mesh_idx = (int)m;
		}
	}
	if (mesh_idx < 0) return;
	const MeshRef& M = S.meshes[mesh_idx];
	int idx;
	float t;
	bvh4_ray_intersect(M.nodes, M.tris, pos, dir, idx, t);
	pos = add3(pos, scale3(dir, t));
	if (idx > -1) {
		const Triangle& tri = M.tris[idx];
		f3 a = ld3(tri.a);
		dir = normalize3(cross3(sub3(ld3(tri.b), a), sub3(ld3(tri.c), a)));
		hit = true;
		if constexpr (WITH_ID) *mesh_id = mesh_idx;
	}
}

// the closest triangle hit of a ray over ALL meshes (trace_mesh's rule is another: one mesh, chosen by box entry): its t, +inf without a
// hit. mesh / tri (nullable) receive the hit's mesh and triangle; they are left alone without a hit. What the irradiance ray generators see.
// S by value: through a reference the compiler no longer sees that the mesh table is global memory and reads the BVHs with flat loads.
NGP_DEV float closest_hit(const MeshSceneParams S, f3 org, f3 dir, int* mesh = nullptr, int* tri = nullptr) {
	float t_max = __builtin_huge_valf();
	for (uint32_t m = 0; m < S.n_meshes; ++m) {
		int idx;
		float t;
		bvh4_ray_intersect(S.meshes[m].nodes, S.meshes[m].tris, org, dir, idx, t);
		if (idx > -1 && t < t_max) {
			t_max = t;
			if (mesh) *mesh = (int)m;
			if (tri) *tri = idx;
		}
	}
	return t_max;
}

// ---- BRDF: testbed_geometry_training.cu:46-144 (double-typed literals are kept, they promote like the reference)
NGP_DEV float square(float x) { return x * x; }
NGP_DEV float mixf(float a, float b, float t) { return a + (b - a) * t; }
NGP_DEV f3 mix3(f3 a, f3 b, float t) { return add3(a, scale3(sub3(b, a), t)); }
NGP_DEV float saturate(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }
NGP_DEV float SchlickFresnel(float u) {
	float m = saturate((float)(1.0 - u));
	return square(square(m)) * m;
}
constexpr float PI_F = 3.14159265358979323846f;
NGP_DEV float G1(float NdotH, float a) {
	if (a >= 1.0) return (float)(1.0 / PI_F);
	float a2 = square(a);
	float t = (float)(1.0 + (a2 - 1.0) * NdotH * NdotH);
	return (float)((a2 - 1.0) / (PI_F * logf(a2) * t));
}
NGP_DEV float G2(float NdotH, float a) {
	float a2 = square(a);
	float t = (float)(1.0 + (a2 - 1.0) * NdotH * NdotH);
	return a2 / (PI_F * t * t);
}
NGP_DEV float SmithG_GGX(float NdotV, float alphaG) {
	float a = alphaG * alphaG;
	float b = NdotV * NdotV;
	return (float)(1.0 / (NdotV + __builtin_sqrtf(a + b - a * b)));
}
NGP_DEV f3 evaluate_shading(f3 base_color, f3 ambient_color, f3 light_color, float metallic, float subsurface, float specular, float roughness,
                            float specular_tint, float sheen, float sheen_tint, float clearcoat, float clearcoat_gloss, f3 L, f3 V, f3 N) {
	float NdotL = dot3(N, L);
	float NdotV = dot3(N, V);
	f3 H = normalize3(add3(L, V));
	float NdotH = dot3(N, H);
	float LdotH = dot3(L, H);
	float FL = SchlickFresnel(NdotL), FV = SchlickFresnel(NdotV);
	f3 amb = scale3(ambient_color, mixf(0.2f, FV, metallic));
	amb = mul3(amb, base_color);
	if (NdotL < 0.f || NdotV < 0.f) return amb;
	float luminance = dot3(base_color, mk3(0.3f, 0.6f, 0.1f));
	f3 Ctint = scale3(base_color, 1.f / (luminance + 0.00001f));
	const f3 one = mk3(1.0f, 1.0f, 1.0f);
	f3 Cspec0 = mix3(scale3(scale3(mix3(one, Ctint, specular_tint), specular), 0.08f), base_color, metallic);
	f3 Csheen = mix3(one, Ctint, sheen_tint);
	float Fd90 = 0.5f + 2.0f * LdotH * LdotH * roughness;
	float Fd = mixf(1, Fd90, FL) * mixf(1.f, Fd90, FV);
	float Fss90 = LdotH * LdotH * roughness;
	float Fss = mixf(1.0f, Fss90, FL) * mixf(1.0f, Fss90, FV);
	float ss = 1.25f * (Fss * (1.f / (NdotL + NdotV) - 0.5f) + 0.5f);
	float a = fmaxf(0.001f, square(roughness));
	float Ds = G2(NdotH, a);
	float FH = SchlickFresnel(LdotH);
	f3 Fs = mix3(Cspec0, one, FH);
	float Gs = SmithG_GGX(NdotL, a) * SmithG_GGX(NdotV, a);
	f3 Fsheen = scale3(Csheen, FH * sheen);
	float Dr = G1(NdotH, mixf(0.1f, 0.001f, clearcoat_gloss));
	float Fr = mixf(0.04f, 1.0f, FH);
	float Gr = SmithG_GGX(NdotL, 0.25f) * SmithG_GGX(NdotV, 0.25f);
	float CCs = 0.25f * clearcoat * Gr * Fr * Dr;
	f3 diffuse = add3(scale3(base_color, (float)(1.0f / PI_F) * mixf(Fd, ss, subsurface)), Fsheen);
	f3 brdf = add3(add3(scale3(diffuse, 1.0f - metallic), scale3(Fs, Gs * Ds)), mk3(CCs, CCs, CCs));
	return add3(scale3(mul3(brdf, light_color), NdotL), amb);
}

// ---- NeRF-derived irradiance (definitions: include/ngp_hip.h, ngp_compute_envmap_grid). The lookups keep one fixed
// expression order.
// cell + weight of a coordinate on an axis of n samples sitting at (k + offset) / n: clamped (theta) or periodic (phi)
NGP_DEV void axis_cell(float coord01, uint32_t n, float offset, bool periodic, uint32_t& k0, uint32_t& k1, float& w) {
	float f = coord01 * (float)n - offset;
	float fl = __builtin_floorf(f);
	int i0 = (int)fl, i1 = i0 + 1;
	w = f - fl;
	if (periodic) {
		i0 = ((i0 % (int)n) + (int)n) % (int)n;
		i1 = ((i1 % (int)n) + (int)n) % (int)n;
	} else {
		if (i0 < 0) { i0 = 0; w = 0.0f; }
		if (i1 > (int)n - 1) i1 = (int)n - 1;
		if (i0 > (int)n - 1) i0 = (int)n - 1;
	}
	k0 = (uint32_t)i0; k1 = (uint32_t)i1;
}
// inverse of cylindrical_to_dir_nerf (src/testbed_nerf.cu:1546-1557): px = (1 - z) / 2, py = atan2(y, x) / (2 pi) + 0.5
NGP_DEV void dir_to_cylindrical(f3 n, float& px, float& py) {
	px = (1.0f - n.z) * 0.5f;
	py = atan2f(n.y, n.x) / (2.0f * PI_F) + 0.5f;
}
// bilinear read of one tabulated irradiance map at direction n, in the manner of read_envmap (envmap.cuh:24-50): the
// four texels around the direction, theta clamped, phi periodic
NGP_DEV f3 irradiance_read(const float4* __restrict__ table, uint32_t n_theta, uint32_t n_phi, f3 n) {
	float px, py, wa, wb;
	uint32_t a0, a1, b0, b1;
	dir_to_cylindrical(n, px, py);
	axis_cell(px, n_theta, 0.0f, false, a0, a1, wa);
	axis_cell(py, n_phi, 0.0f, true, b0, b1, wb);
	const float4 t00 = table[(size_t)a0 + (size_t)n_theta * b0], t10 = table[(size_t)a1 + (size_t)n_theta * b0];
	const float4 t01 = table[(size_t)a0 + (size_t)n_theta * b1], t11 = table[(size_t)a1 + (size_t)n_theta * b1];
	const float w00 = (1.0f - wa) * (1.0f - wb), w10 = wa * (1.0f - wb), w01 = (1.0f - wa) * wb, w11 = wa * wb;
	return mk3((w00 * t00.x + w10 * t10.x) + (w01 * t01.x + w11 * t11.x), (w00 * t00.y + w10 * t10.y) + (w01 * t01.y + w11 * t11.y),
	           (w00 * t00.z + w10 * t10.z) + (w01 * t01.z + w11 * t11.z));
}
// one probe (ShadeEnvMap), or the four probes of the grid around the direction of pos - center (ShadeGridEnvMap)
NGP_DEV f3 irradiance_lookup(const IrradianceMap& I, f3 pos, f3 N) {
	if (I.grid_x == 0u) return irradiance_read(I.irradiance, I.n_theta, I.n_phi, N);
	const size_t texels = (size_t)I.n_theta * I.n_phi;
	f3 rel = sub3(pos, mk3(I.center[0], I.center[1], I.center[2]));
	float len = __builtin_sqrtf(dot3(rel, rel));
	f3 dir = len > 0.0f ? mk3(rel.x / len, rel.y / len, rel.z / len) : mk3(0.f, 0.f, 1.f);
	float px, py, wi, wj;
	uint32_t i0, i1, j0, j1;
	dir_to_cylindrical(dir, px, py);
	axis_cell(px, I.grid_x, 0.5f, false, i0, i1, wi);
	axis_cell(py, I.grid_y, 0.5f, true, j0, j1, wj);
	const f3 e00 = irradiance_read(I.irradiance + texels * (i0 + (size_t)I.grid_x * j0), I.n_theta, I.n_phi, N);
	const f3 e10 = irradiance_read(I.irradiance + texels * (i1 + (size_t)I.grid_x * j0), I.n_theta, I.n_phi, N);
	const f3 e01 = irradiance_read(I.irradiance + texels * (i0 + (size_t)I.grid_x * j1), I.n_theta, I.n_phi, N);
	const f3 e11 = irradiance_read(I.irradiance + texels * (i1 + (size_t)I.grid_x * j1), I.n_theta, I.n_phi, N);
	const float w00 = (1.0f - wi) * (1.0f - wj), w10 = wi * (1.0f - wj), w01 = (1.0f - wi) * wj, w11 = wi * wj;
	return mk3((w00 * e00.x + w10 * e10.x) + (w01 * e01.x + w11 * e11.x), (w00 * e00.y + w10 * e10.y) + (w01 * e01.y + w11 * e11.y),
	           (w00 * e00.z + w10 * e10.z) + (w01 * e01.z + w11 * e11.z));
}

// cell and weight of a coordinate on an axis of r probes spanning [lo, hi]: s = clamp((x - lo) / (hi - lo), 0, 1) (r - 1),
// i0 = min(floor(s), r - 2), f = s - i0; an axis of one probe takes no part (i0 = 0, f = 0)
NGP_DEV void volume_axis(float x, float lo, float hi, uint32_t r, uint32_t& i0, float& f) {
	i0 = 0u;
	f = 0.0f;
	if (r < 2u) return;
	const float xc = fminf(fmaxf(x, lo), hi); // (inside the box first: x - lo cannot overflow where hi - lo, which the host checks, does not)
	const float s = saturate((xc - lo) / (hi - lo)) * (float)(r - 1u);
	const float fl = fminf(__builtin_floorf(s), (float)(r - 2u));
	i0 = (uint32_t)fl;
	f = s - fl;
}

// the volume's estimate at (p, n^): the trilinear blend of the live probes (w != 0) among the up to 8 around p, renormalised by their weight
// W, and E(n^) of the blended coefficients; E = 0 where every corner is dead (W = 0). A probe is 7 float4 (112 B, 16-B aligned). The one
// definition: the lookup kernel and the mesh pass's ShadeIrradianceVolume ambient both call it.
NGP_DEV void irradiance_volume_lookup(const IrradianceVolume& V, f3 p, f3 nh, float (&E)[3], float& W) {
	uint32_t i0[3];
	float f[3];
	volume_axis(p.x, V.lo[0], V.hi[0], V.res[0], i0[0], f[0]);
	volume_axis(p.y, V.lo[1], V.hi[1], V.res[1], i0[1], f[1]);
	volume_axis(p.z, V.lo[2], V.hi[2], V.res[2], i0[2], f[2]);
	float c[28];
#pragma unroll
	for (int j = 0; j < 28; ++j) c[j] = 0.f;
	W = 0.f;
#pragma unroll
	for (uint32_t corner = 0; corner < 8u; ++corner) {
		const uint32_t dx = corner & 1u, dy = (corner >> 1) & 1u, dz = corner >> 2;
		const float wgt = (dx ? f[0] : 1.0f - f[0]) * (dy ? f[1] : 1.0f - f[1]) * (dz ? f[2] : 1.0f - f[2]);
		if (wgt == 0.0f) continue; // (also every second probe of an axis of one: its index would lie outside the lattice)
		const size_t g = (i0[0] + dx) + (size_t)V.res[0] * ((i0[1] + dy) + (size_t)V.res[1] * (i0[2] + dz));
		const float4* rec = V.sh + 7 * g;
		const float4 last = rec[6];
		if (last.w == 0.0f) continue; // a dead probe: every ray blocked
#pragma unroll
		for (int q = 0; q < 6; ++q) {
			const float4 x = rec[q];
			c[4 * q] += wgt * x.x; c[4 * q + 1] += wgt * x.y; c[4 * q + 2] += wgt * x.z; c[4 * q + 3] += wgt * x.w;
		}
		c[24] += wgt * last.x; c[25] += wgt * last.y; c[26] += wgt * last.z;
		W += wgt;
	}
	E[0] = E[1] = E[2] = 0.f;
	if (W > 0.0f) {
		const float inv = 1.0f / W;
#pragma unroll
		for (int j = 0; j < 27; ++j) c[j] *= inv;
		sh9_irradiance(c, nh.x, nh.y, nh.z, E);
	}
}

// ---- visibility-weighted lookup (contract: include/ngp_hip.h, "probe visibility"). A probe's distance map is 8 x 8 octahedral texels of
// (m1, m2), texel q = i + 8 j.
// the direction of texel q: (a, b) = the texel centre in [-1, 1]^2, z = 1 - |a| - |b|, the lower half folded over the diagonals
NGP_DEV f3 distance_texel_dir(uint32_t q) {
	const float a = 2.0f * ((float)(q & 7u) + 0.5f) / 8.0f - 1.0f, b = 2.0f * ((float)(q >> 3) + 0.5f) / 8.0f - 1.0f;
	const float z = 1.0f - fabsf(a) - fabsf(b);
	float x = a, y = b;
	if (z < 0.0f) {
		x = (1.0f - fabsf(b)) * (a < 0.0f ? -1.0f : 1.0f);
		y = (1.0f - fabsf(a)) * (b < 0.0f ? -1.0f : 1.0f);
	}
	return normalize3(mk3(x, y, z));
}
// texel (i, j) of a map, i and j in -1..8: an index outside 0..7 continues across the octahedron's edge
NGP_DEV float2 distance_map_texel(const float2* __restrict__ map, int i, int j) {
	if (i < 0) { i = -1 - i; j = 7 - j; }
	else if (i > 7) { i = 15 - i; j = 7 - j; }
	if (j < 0) { j = -1 - j; i = 7 - i; }
	else if (j > 7) { j = 15 - j; i = 7 - i; }
	return map[i + 8 * j];
}
// bilinear read of a map at the unit direction d: the inverse of distance_texel_dir, then the four texels around (s, t)
NGP_DEV float2 distance_map_read(const float2* __restrict__ map, f3 d) {
	const float inv = 1.0f / (fabsf(d.x) + fabsf(d.y) + fabsf(d.z));
	float a = d.x * inv, b = d.y * inv;
	if (d.z < 0.0f) {
		const float fa = (1.0f - fabsf(b)) * (a < 0.0f ? -1.0f : 1.0f), fb = (1.0f - fabsf(a)) * (b < 0.0f ? -1.0f : 1.0f);
		a = fa;
		b = fb;
	}
	const float s = 4.0f * (a + 1.0f) - 0.5f, t = 4.0f * (b + 1.0f) - 0.5f;
	const float fs = __builtin_floorf(s), ft = __builtin_floorf(t);
	const int i0 = min(max((int)fs, -1), 7), j0 = min(max((int)ft, -1), 7); // (|a|, |b| <= 1 up to rounding: the clamp keeps every read inside the map)
	const float ws = s - fs, wt = t - ft;
	const float2 t00 = distance_map_texel(map, i0, j0), t10 = distance_map_texel(map, i0 + 1, j0);
	const float2 t01 = distance_map_texel(map, i0, j0 + 1), t11 = distance_map_texel(map, i0 + 1, j0 + 1);
	const float w00 = (1.0f - ws) * (1.0f - wt), w10 = ws * (1.0f - wt), w01 = (1.0f - ws) * wt, w11 = ws * wt;
	return make_float2((w00 * t00.x + w10 * t10.x) + (w01 * t01.x + w11 * t11.x), (w00 * t00.y + w10 * t10.y) + (w01 * t01.y + w11 * t11.y));
}
// position of probe i on an axis of r probes over [lo, hi], as the host places it: in double, rounded to float
NGP_DEV float volume_probe_coord(float lo, float hi, uint32_t r, uint32_t i) {
	const double frac = r > 1u ? (double)i / (double)(r - 1u) : 0.5;
	return (float)((double)lo + frac * ((double)hi - (double)lo));
}

// irradiance_volume_lookup with every live corner's weight multiplied by the Chebyshev visibility of the point from that probe: cells, weights
// and the order of operations are the plain lookup's, so vis = 1 at every corner gives its bits. The one definition: the visible lookup
// kernel and the mesh pass's third instantiation both call it.
NGP_DEV void irradiance_volume_lookup_visible(const IrradianceVolumeVisible& A, f3 p, f3 nh, float (&E)[3], float& W) {
	const IrradianceVolume& V = A.V;
	uint32_t i0[3];
	float f[3];
	volume_axis(p.x, V.lo[0], V.hi[0], V.res[0], i0[0], f[0]);
	volume_axis(p.y, V.lo[1], V.hi[1], V.res[1], i0[1], f[1]);
	volume_axis(p.z, V.lo[2], V.hi[2], V.res[2], i0[2], f[2]);
	const f3 pb = add3(p, scale3(nh, A.normal_bias));
	const float var_floor = 1e-4f * A.D * A.D;
	float c[28];
#pragma unroll
	for (int j = 0; j < 28; ++j) c[j] = 0.f;
	W = 0.f;
#pragma unroll
	for (uint32_t corner = 0; corner < 8u; ++corner) {
		const uint32_t dx = corner & 1u, dy = (corner >> 1) & 1u, dz = corner >> 2;
		const float wgt = (dx ? f[0] : 1.0f - f[0]) * (dy ? f[1] : 1.0f - f[1]) * (dz ? f[2] : 1.0f - f[2]);
		if (wgt == 0.0f) continue;
		const size_t g = (i0[0] + dx) + (size_t)V.res[0] * ((i0[1] + dy) + (size_t)V.res[1] * (i0[2] + dz));
		const float4* rec = V.sh + 7 * g;
		const float4 last = rec[6];
		if (last.w == 0.0f) continue; // a dead probe
		const f3 v = sub3(pb, mk3(volume_probe_coord(V.lo[0], V.hi[0], V.res[0], i0[0] + dx), volume_probe_coord(V.lo[1], V.hi[1], V.res[1], i0[1] + dy),
		                          volume_probe_coord(V.lo[2], V.hi[2], V.res[2], i0[2] + dz)));
		const float r = __builtin_sqrtf(dot3(v, v));
		float vis = 1.0f;
		if (r > 0.0f) {
			const float2 m = distance_map_read(A.maps + DISTANCE_MAP_TEXELS * g, mk3(v.x / r, v.y / r, v.z / r));
			if (!(r <= m.x)) {
				const float var = fmaxf(m.y - m.x * m.x, var_floor), d = r - m.x;
				const float ch = var / (var + d * d);
				vis = ch * ch * ch;
			}
		}
		const float wv = wgt * vis;
#pragma unroll
		for (int q = 0; q < 6; ++q) {
			const float4 x = rec[q];
			c[4 * q] += wv * x.x; c[4 * q + 1] += wv * x.y; c[4 * q + 2] += wv * x.z; c[4 * q + 3] += wv * x.w;
		}
		c[24] += wv * last.x; c[25] += wv * last.y; c[26] += wv * last.z;
		W += wv;
	}
	E[0] = E[1] = E[2] = 0.f;
	if (W > 0.0f) {
		const float inv = 1.0f / W;
#pragma unroll
		for (int j = 0; j < 27; ++j) c[j] *= inv;
		sh9_irradiance(c, nh.x, nh.y, nh.z, E);
	}
}

// ---- the frames' mesh pass: render_geometry_mesh (src/testbed_geometry_training.cu:2202-2320), Shade mode, floor disabled, one thread per
// pixel (frame_pixel, render_common.h). Its stages M1-M5 are the three functions below, the one definition of each: render_mesh_fused runs
// them back to back, the split pass (mesh_gbuffer_kernel, mesh_shade_deferred_kernel) runs the same functions in the same order around the
// ray-list traces, so a split-pass pixel whose T_s is 1 gets the fused kernel's bits.
// The three take the kernels' parameter structs by value, as closest_hit does: through references the fused kernel reloads twice as many
// spilled scalar registers and its pass measures 3 us longer.
NGP_DEV void st3(float* p, f3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
NGP_DEV f3 shadow_ray_dir(const MeshShadeParams& P) { return normalize3(normalize3(ld3(P.sun_dir))); } // (M3 normalises m_sun_dir twice)
NGP_DEV float camera_depth(const CameraParams& C, f3 pos) { return dot3(mk3(C.m[6], C.m[7], C.m[8]), sub3(pos, mk3(C.m[9], C.m[10], C.m[11]))); }

// M1: init_rays_with_payload_kernel_mesh_geometry (:488-579): pixel (x, y)'s ray through the lens and the aperture, advanced to the scene
// box: pos, and the unit dir. false: the lens gives the pixel no direction (it keeps MAX_DEPTH and an empty frame)
NGP_DEV bool mesh_primary_ray(const MeshSceneParams S, const CameraParams C, uint32_t x, uint32_t y, f3& pos, f3& dir) {
	float u = ((float)x + C.pixel_offset[0]) / (float)C.width;
	float v = ((float)y + C.pixel_offset[1]) / (float)C.height;
	lens_direction(C, u, v, dir);
	dir = m3_mulv(C.m, dir);
	f3 origin = mk3(C.m[9], C.m[10], C.m[11]);
	if (C.aperture_size != 0.0f) {
		float o3[3] = {origin.x, origin.y, origin.z}, d3[3] = {dir.x, dir.y, dir.z}, cm[6];
		for (int i = 0; i < 6; ++i) cm[i] = C.m[i];
		apply_aperture(cm, C.aperture_size, C.focus_z, C.spp, (uint32_t)(int)(u * (float)C.width) * 19349663u + (uint32_t)(int)(v * (float)C.height) * 96925573u, o3, d3);
		origin = mk3(o3[0], o3[1], o3[2]);
		dir = mk3(d3[0], d3[1], d3[2]);
	}
	origin = add3(origin, scale3(dir, C.near_distance));
	if (dir.x == 0.0f && dir.y == 0.0f && dir.z == 0.0f) return false;
	dir = normalize3(dir);
	float t = fmaxf(aabb_ray_entry(S.scene_min, S.scene_max, origin, dir), 0.0f);
	pos = add3(origin, scale3(dir, t + 1e-6f));
	return true;
}

// M2 on every ray (the normal buffer starts out holding the ray direction, trace_mesh_bvh :2140-2155), M3 prepare_shadow_rays_geometry
// (:222-271) and M4 write_shadow_ray_result_geometry (:273-278, min_visibility == 1). pos: the primary ray's start in, its end out; hit: it
// found a triangle; q: where the shadow ray leaves the surface, before M3 advances it to the scene box (the split pass starts the NeRF's
// shadow ray and the mirror ray there); shadow: 1 where no mesh stands between q and the sun, else 0.
// WITH_ID: *mesh_id receives the mesh of the primary hit, -1 without one (geometry never depends on a material: nothing else changes).
template <bool WITH_ID = false>
NGP_DEV void mesh_trace_shadow(const MeshSceneParams S, const MeshShadeParams P, f3 primary_dir, f3& pos, f3& normal, bool& hit, f3& q, float& shadow, int* mesh_id = nullptr) {
	normal = primary_dir;
	trace_mesh<WITH_ID>(S, pos, normal, hit, mesh_id);
	const f3 sdir = shadow_ray_dir(P);
	float nd = dot3(normal, primary_dir);
	f3 ff = nd < 0.0f ? normal : scale3(normal, -1.0f); // faceforward(n, dir, n)
	f3 view_pos = add3(pos, scale3(normalize3(ff), 1e-3f));
	q = view_pos;
	float st = fmaxf(aabb_ray_entry(S.scene_min, S.scene_max, view_pos, sdir) + 1e-6f, 0.0f);
	view_pos = add3(view_pos, scale3(sdir, st));
	f3 spos = view_pos;
	f3 sn = box_contains(S.scene_min, S.scene_max, view_pos) ? sdir : primary_dir; // dead shadow rays keep the copied payload.dir
	bool shadow_hit;
	trace_mesh(S, spos, sn, shadow_hit);
	shadow = box_contains(S.scene_min, S.scene_max, spos) ? 0.0f : 1.0f;
}

// the material a shade at mesh m uses (contract: include/ngp_hip.h, "mesh materials"): the mesh's own record where it owns one, else the
// context's P; the sun and up directions are P's either way. m = -1 (no triangle: the pixel shaded at the camera): P.
NGP_DEV MeshShadeParams mesh_material_of(const MeshShadeParams P, const MeshMaterial* __restrict__ table, int m) {
	MeshShadeParams Q = P;
	if (m < 0) return Q;
	const float4* rec = reinterpret_cast<const float4*>(table + m);
	const float4 a = rec[0], b = rec[1], c = rec[2], d = rec[3];
	if (__float_as_uint(d.y) == 0u) return Q;
	Q.metallic = a.x; Q.subsurface = a.y; Q.specular = a.z; Q.roughness = a.w;
	Q.sheen = b.x; Q.clearcoat = b.y; Q.clearcoat_gloss = b.z;
	Q.basecolor[0] = b.w; Q.basecolor[1] = c.x; Q.basecolor[2] = c.y;
	Q.ambientcolor[0] = c.z; Q.ambientcolor[1] = c.w; Q.ambientcolor[2] = d.x;
	return Q;
}

// M5: shade_kernel_mesh_geometry (:280-355) at a covered pixel. The ambient source is fixed at compile time by the type of A: IrradianceMap
// (the sky term, or the probe table(s) when A.irradiance is set), IrradianceVolume (ShadeIrradianceVolume: max(E(pos, N), 0) / pi from the
// SH9 lattice, 0 where every probe around pos is dead) or IrradianceVolumeVisible (the same mode while the context holds the probes'
// distance maps: the visibility-weighted estimate).
template <typename Ambient>
NGP_DEV f3 mesh_shade(const MeshShadeParams P, const Ambient A, f3 pos, f3 normal, f3 primary_dir, float shadow) {
	const f3 sun = normalize3(ld3(P.sun_dir));
	f3 N = normalize3(normal);
	f3 up = normalize3(ld3(P.up_dir));
	float skyam = -dot3(N, up) * 0.5f + 0.5f;
	f3 suncol = scale3(scale3(mk3(255.f / 255.0f, 225.f / 255.0f, 195.f / 255.0f), 4.f), shadow);
	f3 skycol = scale3(scale3(mk3(195.f / 255.0f, 215.f / 255.0f, 255.f / 255.0f), 4.f), skyam);
	f3 base = ld3(P.basecolor);
	f3 ambc;
	if constexpr (std::is_same<Ambient, IrradianceMap>::value) {
		ambc = mul3(ld3(P.ambientcolor), skycol);
		if (A.irradiance) { // ShadeEnvMap / ShadeGridEnvMap: ambient light = E(N)/pi from the NeRF-derived irradiance table(s)
			f3 E = irradiance_lookup(A, pos, N);
			ambc = mk3(E.x / PI_F, E.y / PI_F, E.z / PI_F);
		}
	} else { // the blend's accumulators are live from here on only: both traversals are over
		float E[3], W;
		if constexpr (std::is_same<Ambient, IrradianceVolume>::value) irradiance_volume_lookup(A, pos, N, E, W);
		else irradiance_volume_lookup_visible(A, pos, N, E, W);
		ambc = mk3(fmaxf(E[0], 0.0f) / PI_F, fmaxf(E[1], 0.0f) / PI_F, fmaxf(E[2], 0.0f) / PI_F); // (SH9 rings: E may dip below zero)
	}
	return evaluate_shading(mul3(base, base), ambc, suncol, P.metallic, P.subsurface, P.specular, P.roughness, 0.f, P.sheen, 0.f, P.clearcoat, P.clearcoat_gloss, sun,
	                        scale3(normalize3(primary_dir), -1.0f), N);
}

// the whole pass in one kernel: primary hit, sun shadow ray and BRDF stay in registers
template <typename Ambient>
__global__ void render_mesh_fused(const MeshSceneParams S, const MeshShadeParams P, const Ambient A, const CameraParams C, const FrameLayout L,
                                  float4* __restrict__ frame_buffer, float* __restrict__ depth_buffer) {
	uint32_t x, y, idx;
	if (!frame_pixel(L, C, x, y, idx)) return;
	depth_buffer[idx] = MAX_DEPTH;
	f3 pos, primary_dir, normal, q;
	if (!mesh_primary_ray(S, C, x, y, pos, primary_dir)) return;
	bool hit;
	float shadow;
	mesh_trace_shadow(S, P, primary_dir, pos, normal, hit, q, shadow);
	if (!box_contains(S.scene_min, S.scene_max, pos)) return;
	f3 color = mesh_shade(P, A, pos, normal, primary_dir, shadow);
	frame_buffer[idx] = make_float4(color.x, color.y, color.z, 1.0f);
	depth_buffer[idx] = camera_depth(C, pos);
}

// render_mesh_fused with materials: the same stages, M5 with the material of the mesh the primary ray hit. ids: the frame's id plane, the mesh
// of the primary hit, -1 on every other pixel (ngp_get_frame_mesh_ids)
template <typename Ambient>
__global__ void render_mesh_fused_materials(const MeshSceneParams S, const MeshShadeParams P, const Ambient A, const CameraParams C, const FrameLayout L,
                                            float4* __restrict__ frame_buffer, float* __restrict__ depth_buffer, const MeshMaterial* __restrict__ materials,
                                            int32_t* __restrict__ ids) {
	uint32_t x, y, idx;
	if (!frame_pixel(L, C, x, y, idx)) return;
	depth_buffer[idx] = MAX_DEPTH;
	ids[idx] = -1;
	f3 pos, primary_dir, normal, q;
	if (!mesh_primary_ray(S, C, x, y, pos, primary_dir)) return;
	bool hit;
	float shadow;
	int mesh;
	mesh_trace_shadow<true>(S, P, primary_dir, pos, normal, hit, q, shadow, &mesh);
	if (!box_contains(S.scene_min, S.scene_max, pos)) return;
	ids[idx] = mesh;
	f3 color = mesh_shade(mesh_material_of(P, materials, mesh), A, pos, normal, primary_dir, shadow);
	frame_buffer[idx] = make_float4(color.x, color.y, color.z, 1.0f);
	depth_buffer[idx] = camera_depth(C, pos);
}

// stage kernel: M2 alone (mesh_raytrace_kernel)
__global__ void trace_mesh_rays_kernel(const MeshSceneParams S, uint32_t n, float* __restrict__ positions, float* __restrict__ directions) {
	uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	f3 p = ld3(positions + 3 * (size_t)i), d = ld3(directions + 3 * (size_t)i);
	bool hit;
	trace_mesh(S, p, d, hit);
	st3(positions + 3 * (size_t)i, p);
	st3(directions + 3 * (size_t)i, d);
}

// ---- the split pass (ngp_set_sun_nerf_shadow, ngp_set_mesh_reflection; contracts in include/ngp_hip.h, "sun: the NeRF in front of the
// frames' sun" and "mesh reflection"): M1-M4 leave a G-buffer and one shadow-ray entry per local pixel, in idx order and not compacted; the
// tracer walks the list(s); M5 shades from the G-buffer with shadow scaled by what the tracer let through.
// G-buffer of n pixels, three planes of n float4: (pos, shadow), (raw normal, covered), (primary_dir, the primary ray found a triangle).
// IDS (the material instantiation): the int32 id plane beside the G-buffer receives the mesh of the primary hit, -1 on every other pixel.
template <bool IDS>
NGP_DEV void mesh_gbuffer_body(const MeshSceneParams S, const MeshShadeParams P, const CameraParams C, const FrameLayout L, float* __restrict__ depth_buffer, float t_min,
                               float4* __restrict__ gbuf, float* __restrict__ ray_o, float* __restrict__ ray_d, float2* __restrict__ ray_t, int32_t* __restrict__ ids) {
	uint32_t x, y, idx;
	if (!frame_pixel(L, C, x, y, idx)) return;
	depth_buffer[idx] = MAX_DEPTH;
	if constexpr (IDS) ids[idx] = -1;
	// the dead entry irradiance_sun_shadow_rays_kernel writes: origin 0, the sun's direction, t = (0, 0)
	st3(ray_d + 3 * (size_t)idx, shadow_ray_dir(P));
	f3 pos, primary_dir, normal, q;
	if (!mesh_primary_ray(S, C, x, y, pos, primary_dir)) {
		gbuf[(size_t)L.n_pixels + idx] = make_float4(0.f, 0.f, 0.f, 0.f); // not covered
		st3(ray_o + 3 * (size_t)idx, mk3(0.f, 0.f, 0.f));
		ray_t[idx] = make_float2(0.f, 0.f);
		return;
	}
	bool hit;
	float shadow;
	int mesh = -1;
	mesh_trace_shadow<IDS>(S, P, primary_dir, pos, normal, hit, q, shadow, &mesh);
	const bool covered = box_contains(S.scene_min, S.scene_max, pos);
	if constexpr (IDS) {
		if (covered) ids[idx] = mesh;
	}
	const bool has = covered && shadow == 1.0f; // the NeRF's shadow ray starts at q, where the mesh shadow ray does
	if (!has) q = mk3(0.f, 0.f, 0.f);
	gbuf[idx] = make_float4(pos.x, pos.y, pos.z, shadow);
	gbuf[(size_t)L.n_pixels + idx] = make_float4(normal.x, normal.y, normal.z, covered ? 1.0f : 0.0f);
	gbuf[2 * (size_t)L.n_pixels + idx] = make_float4(primary_dir.x, primary_dir.y, primary_dir.z, hit ? 1.0f : 0.0f);
	st3(ray_o + 3 * (size_t)idx, q);
	ray_t[idx] = has ? make_float2(t_min, __builtin_huge_valf()) : make_float2(0.0f, 0.0f);
	if (covered) depth_buffer[idx] = camera_depth(C, pos);
}
__global__ void mesh_gbuffer_kernel(const MeshSceneParams S, const MeshShadeParams P, const CameraParams C, const FrameLayout L, float* __restrict__ depth_buffer, float t_min,
                                    float4* __restrict__ gbuf, float* __restrict__ ray_o, float* __restrict__ ray_d, float2* __restrict__ ray_t) {
	mesh_gbuffer_body<false>(S, P, C, L, depth_buffer, t_min, gbuf, ray_o, ray_d, ray_t, nullptr);
}
__global__ void mesh_gbuffer_ids_kernel(const MeshSceneParams S, const MeshShadeParams P, const CameraParams C, const FrameLayout L, float* __restrict__ depth_buffer, float t_min,
                                        float4* __restrict__ gbuf, float* __restrict__ ray_o, float* __restrict__ ray_d, float2* __restrict__ ray_t, int32_t* __restrict__ ids) {
	mesh_gbuffer_body<true>(S, P, C, L, depth_buffer, t_min, gbuf, ray_o, ray_d, ray_t, ids);
}

// the mirror ray of a G-buffer pixel, in one fixed order: n^ = normalize(ff), ff M3's winding normal turned against the primary ray;
// c = -(n^ . primary_dir); q = pos + 1e-3 n^ (M3's view_pos, the shadow list's q, as bits); r = primary_dir + (2 c) n^, not normalised
NGP_DEV void mirror_ray(f3 pos, f3 normal, f3 primary_dir, f3& q, f3& r, float& c) {
	float nd = dot3(normal, primary_dir);
	f3 ff = nd < 0.0f ? normal : scale3(normal, -1.0f);
	f3 nh = normalize3(ff);
	c = -dot3(nh, primary_dir);
	q = add3(pos, scale3(nh, 1e-3f));
	r = add3(primary_dir, scale3(nh, 2.0f * c));
}

// what a pixel's mirror ray adds to its colour: strength F (.) rgb_r, F = mix3(Cspec0, 1, SchlickFresnel(c)), Cspec0 the BRDF's with its tint at 0
NGP_DEV f3 mirror_term(const MeshShadeParams& P, float c, f3 rgb_r, float strength) {
	const f3 one = mk3(1.0f, 1.0f, 1.0f);
	f3 base = ld3(P.basecolor);
	f3 Cspec0 = mix3(scale3(scale3(one, P.specular), 0.08f), mul3(base, base), P.metallic);
	f3 F = mix3(Cspec0, one, SchlickFresnel(c));
	return scale3(mul3(F, rgb_r), strength);
}

// the pixel's entry of the reflection list, in idx order and not compacted. A pixel owns a ray where it is covered and its primary ray found
// a triangle (plane 2's w); t = (t_min, the closest triangle over ALL meshes from q along normalize(r), +inf without one), ngp_irradiance_rays'
// rule. Every other entry is dead: origin 0, direction +z, t = (0, 0). hit_ids (nullable: ngp_set_mesh_reflection_meshes is off) receives the
// (mesh, triangle) of that closest hit, (-1, -1) where the pixel owns no ray or its ray is not cut.
__global__ void mesh_reflection_rays_kernel(const MeshSceneParams S, const CameraParams C, const FrameLayout L, float t_min, const float4* __restrict__ gbuf,
                                            float* __restrict__ ray_o, float* __restrict__ ray_d, float2* __restrict__ ray_t, int2* __restrict__ hit_ids) {
	uint32_t x, y, idx;
	if (!frame_pixel(L, C, x, y, idx)) return;
	f3 q = mk3(0.f, 0.f, 0.f), r = mk3(0.f, 0.f, 1.f);
	float2 t = make_float2(0.f, 0.f);
	int mesh = -1, tri = -1;
	const float4 g1 = gbuf[(size_t)L.n_pixels + idx];
	if (g1.w != 0.0f) { // (a pixel that is not covered may hold a stale plane 2)
		const float4 g2 = gbuf[2 * (size_t)L.n_pixels + idx];
		if (g2.w != 0.0f) {
			const float4 g0 = gbuf[idx];
			float c;
			mirror_ray(mk3(g0.x, g0.y, g0.z), mk3(g1.x, g1.y, g1.z), mk3(g2.x, g2.y, g2.z), q, r, c);
			t = make_float2(t_min, closest_hit(S, q, normalize3(r), &mesh, &tri));
		}
	}
	st3(ray_o + 3 * (size_t)idx, q);
	st3(ray_d + 3 * (size_t)idx, r);
	ray_t[idx] = t;
	if (hit_ids) hit_ids[idx] = make_int2(mesh, tri);
}

// M5 from the G-buffer. traced (nullable: no shadow trace was run, T_s = 1): the tracer's rgba of the pixel's list entry; a pixel has a shadow
// ray where ray_t.y != 0 (the prep step moves ray_t.x alone). record: (q, alpha_s), zeros without a shadow ray (ngp_get_frame_sun_shadow).
// R: the mirror ray's radiance is added behind evaluate_shading where alpha_r > 0; every other pixel keeps its bits. With R.hits
// (ngp_set_mesh_reflection_meshes) a ray that a mesh cuts carries L = rgb_r + max(1 - alpha_r, 0) C2, C2 the hit's own M5 from
// mesh_reflection_hit_shade_kernel, and adds it whatever alpha_r is; a ray without a hit keeps the bits it has with R.hits null.
// MAT (the material instantiation): M5 and mirror_term's F take the material of the pixel's mesh in the id plane (mesh_material_of).
template <bool MAT, typename Ambient>
NGP_DEV void mesh_shade_deferred_body(const MeshShadeParams P0, const Ambient A, const CameraParams C, const FrameLayout L, float4* __restrict__ frame_buffer,
                                      const float4* __restrict__ gbuf, const float* __restrict__ ray_o, const float2* __restrict__ ray_t,
                                      const float4* __restrict__ traced, float4* __restrict__ record, const MeshReflectionList R,
                                      const MeshMaterial* __restrict__ materials, const int32_t* __restrict__ ids) {
	uint32_t x, y, idx;
	if (!frame_pixel(L, C, x, y, idx)) return;
	const float4 g1 = gbuf[(size_t)L.n_pixels + idx];
	const bool has = traced && g1.w != 0.0f && ray_t[idx].y != 0.0f;
	const float alpha_s = has ? traced[idx].w : 0.0f;
	if (traced) record[idx] = has ? make_float4(ray_o[3 * (size_t)idx], ray_o[3 * (size_t)idx + 1], ray_o[3 * (size_t)idx + 2], alpha_s) : make_float4(0.f, 0.f, 0.f, 0.f);
	// a pixel owns a mirror ray by mesh_reflection_rays_kernel's rule: covered, and its primary ray found a triangle
	const bool mirror = R.traced && g1.w != 0.0f && gbuf[2 * (size_t)L.n_pixels + idx].w != 0.0f;
	if (R.traced && !mirror) R.record[3 * (size_t)idx] = R.record[3 * (size_t)idx + 1] = R.record[3 * (size_t)idx + 2] = make_float4(0.f, 0.f, 0.f, 0.f);
	if (g1.w == 0.0f) return;
	const float4 g0 = gbuf[idx], g2 = gbuf[2 * (size_t)L.n_pixels + idx];
	const f3 pos = mk3(g0.x, g0.y, g0.z), normal = mk3(g1.x, g1.y, g1.z), primary_dir = mk3(g2.x, g2.y, g2.z);
	float shadow = g0.w;
	if (has) shadow = shadow * fmaxf(1.0f - alpha_s, 0.0f); // T_s
	MeshShadeParams P = P0;
	if constexpr (MAT) P = mesh_material_of(P0, materials, ids[idx]);
	f3 color = mesh_shade(P, A, pos, normal, primary_dir, shadow);
	if (mirror) {
		f3 q, r;
		float c;
		mirror_ray(pos, normal, primary_dir, q, r, c); // (the list's bits: one device function forms them in both kernels)
		const float4 tr = R.traced[idx];
		R.record[3 * (size_t)idx] = make_float4(R.ray_o[3 * (size_t)idx], R.ray_o[3 * (size_t)idx + 1], R.ray_o[3 * (size_t)idx + 2], R.ray_t[idx].y);
		R.record[3 * (size_t)idx + 1] = make_float4(r.x, r.y, r.z, 0.0f);
		R.record[3 * (size_t)idx + 2] = tr;
		f3 Lr = mk3(tr.x, tr.y, tr.z);
		bool cut = false; // the ray owns a shaded mesh hit: its colour stands behind the NeRF along the ray
		if (R.hits) {
			const float4 h1 = R.hits[2 * (size_t)idx + 1];
			cut = h1.w != 0.0f;
			if (cut) Lr = add3(Lr, scale3(mk3(h1.x, h1.y, h1.z), fmaxf(1.0f - tr.w, 0.0f)));
		}
		if (tr.w > 0.0f || cut) color = add3(color, mirror_term(P, c, Lr, R.strength));
	}
	frame_buffer[idx] = make_float4(color.x, color.y, color.z, 1.0f);
}
template <typename Ambient>
__global__ void mesh_shade_deferred_kernel(const MeshShadeParams P, const Ambient A, const CameraParams C, const FrameLayout L, float4* __restrict__ frame_buffer,
                                           const float4* __restrict__ gbuf, const float* __restrict__ ray_o, const float2* __restrict__ ray_t,
                                           const float4* __restrict__ traced, float4* __restrict__ record, const MeshReflectionList R) {
	mesh_shade_deferred_body<false>(P, A, C, L, frame_buffer, gbuf, ray_o, ray_t, traced, record, R, nullptr, nullptr);
}
template <typename Ambient>
__global__ void mesh_shade_deferred_materials_kernel(const MeshShadeParams P, const Ambient A, const CameraParams C, const FrameLayout L, float4* __restrict__ frame_buffer,
                                                     const float4* __restrict__ gbuf, const float* __restrict__ ray_o, const float2* __restrict__ ray_t,
                                                     const float4* __restrict__ traced, float4* __restrict__ record, const MeshReflectionList R,
                                                     const MeshMaterial* __restrict__ materials, const int32_t* __restrict__ ids) {
	mesh_shade_deferred_body<true>(P, A, C, L, frame_buffer, gbuf, ray_o, ray_t, traced, record, R, materials, ids);
}

// the launch geometry of every frame_pixel kernel: blocks of 16 x 8 threads over the camera
static dim3 pixel_threads() { return dim3(16, 8, 1); }
static dim3 pixel_blocks(const CameraParams& C) { return dim3((C.width + 15) / 16, (C.height + 7) / 8, 1); }
// calls f with the ambient source of a mesh shade. VV != nullptr: the SH9 volume weighted by its probes' visibility, and neither V nor I is
// looked at; else V != nullptr: the volume (ShadeIrradianceVolume), and I is not looked at; else I
template <typename F>
void with_ambient(const IrradianceMap& I, const IrradianceVolume* V, const IrradianceVolumeVisible* VV, F&& f) {
	if (VV) f(*VV);
	else if (V) f(*V);
	else f(I);
}

void launch_render_mesh(const MeshSceneParams& S, const MeshShadeParams& P, const IrradianceMap& I, const IrradianceVolume* V, const IrradianceVolumeVisible* VV,
                        const CameraParams& C, const FrameLayout& L, float4* frame_buffer, float* depth_buffer, const MeshMaterial* materials, int32_t* ids, hipStream_t stream) {
	with_ambient(I, V, VV, [&](const auto& A) {
		if (materials)
			hipLaunchKernelGGL(HIP_KERNEL_NAME(render_mesh_fused_materials<std::decay_t<decltype(A)>>), pixel_blocks(C), pixel_threads(), 0, stream, S, P, A, C, L, frame_buffer,
			                   depth_buffer, materials, ids);
		else hipLaunchKernelGGL(HIP_KERNEL_NAME(render_mesh_fused<std::decay_t<decltype(A)>>), pixel_blocks(C), pixel_threads(), 0, stream, S, P, A, C, L, frame_buffer, depth_buffer);
	});
}
// the two halves of launch_render_mesh around the caller's trace of (ray_o, ray_d, ray_t)
void launch_mesh_gbuffer(const MeshSceneParams& S, const MeshShadeParams& P, const CameraParams& C, const FrameLayout& L, float* depth_buffer, float t_min, float4* gbuf,
                         float* ray_o, float* ray_d, float2* ray_t, int32_t* ids, hipStream_t stream) {
	if (ids) hipLaunchKernelGGL(mesh_gbuffer_ids_kernel, pixel_blocks(C), pixel_threads(), 0, stream, S, P, C, L, depth_buffer, t_min, gbuf, ray_o, ray_d, ray_t, ids);
	else hipLaunchKernelGGL(mesh_gbuffer_kernel, pixel_blocks(C), pixel_threads(), 0, stream, S, P, C, L, depth_buffer, t_min, gbuf, ray_o, ray_d, ray_t);
}
void launch_mesh_shade_deferred(const MeshShadeParams& P, const IrradianceMap& I, const IrradianceVolume* V, const IrradianceVolumeVisible* VV, const CameraParams& C,
                                const FrameLayout& L, float4* frame_buffer, const float4* gbuf, const float* ray_o, const float2* ray_t, const float4* traced, float4* record,
                                const MeshReflectionList& R, const MeshMaterial* materials, const int32_t* ids, hipStream_t stream) {
	with_ambient(I, V, VV, [&](const auto& A) {
		if (materials)
			hipLaunchKernelGGL(HIP_KERNEL_NAME(mesh_shade_deferred_materials_kernel<std::decay_t<decltype(A)>>), pixel_blocks(C), pixel_threads(), 0, stream, P, A, C, L, frame_buffer,
			                   gbuf, ray_o, ray_t, traced, record, R, materials, ids);
		else
			hipLaunchKernelGGL(HIP_KERNEL_NAME(mesh_shade_deferred_kernel<std::decay_t<decltype(A)>>), pixel_blocks(C), pixel_threads(), 0, stream, P, A, C, L, frame_buffer, gbuf, ray_o,
			                   ray_t, traced, record, R);
	});
}
void launch_mesh_reflection_rays(const MeshSceneParams& S, const CameraParams& C, const FrameLayout& L, float t_min, const float4* gbuf, float* ray_o, float* ray_d,
                                 float2* ray_t, int2* hit_ids, hipStream_t stream) {
	hipLaunchKernelGGL(mesh_reflection_rays_kernel, pixel_blocks(C), pixel_threads(), 0, stream, S, C, L, t_min, gbuf, ray_o, ray_d, ray_t, hit_ids);
}

// stage kernel: the irradiance lookup at explicit surface points (ngp_irradiance_at)
__global__ void irradiance_lookup_kernel(const IrradianceMap I, uint32_t n, const float* __restrict__ positions, const float* __restrict__ normals, float4* __restrict__ out) {
	uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	f3 E = irradiance_lookup(I, ld3(positions + 3 * (size_t)i), ld3(normals + 3 * (size_t)i));
	out[i] = make_float4(E.x, E.y, E.z, 0.f);
}
void launch_irradiance_lookup(const IrradianceMap& I, uint32_t n, const float* positions, const float* normals, float4* out, hipStream_t stream) {
	if (n) hipLaunchKernelGGL(irradiance_lookup_kernel, dim3((n + 127) / 128), dim3(128), 0, stream, I, n, positions, normals, out);
}
void launch_trace_mesh_rays(const MeshSceneParams& S, uint32_t n, float* positions, float* directions, hipStream_t stream) {
	hipLaunchKernelGGL(trace_mesh_rays_kernel, dim3((n + 127) / 128), dim3(128), 0, stream, S, n, positions, directions);
}


// ---- traced irradiance (ngp_trace_nerf_rays, ngp_irradiance_rays, ngp_irradiance_traced; contract in include/ngp_hip.h).
// The ray list feeds the probe tracer (ProbeParams mode PROBE_RAY_LIST); generator, BVH and reduction stay out of the fused kernel.

// t[i] = (t_min, t_max) -> (t_start, t_max): t_start = max(t_min, the render box's entry distance + 1e-6 as for camera rays, 0 for an
// origin inside the box); a ray that misses the box is dead (t_start = t_max). normalize: the caller's directions are normalised first.
__global__ void ray_list_prep_kernel(const ModelParams M, uint32_t n, const float* __restrict__ o, float* __restrict__ d, float2* __restrict__ t, int normalize) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const f3 org = ld3(o + 3 * (size_t)i);
	f3 dir = ld3(d + 3 * (size_t)i);
	if (normalize) {
		dir = normalize3(dir);
		d[3 * (size_t)i] = dir.x; d[3 * (size_t)i + 1] = dir.y; d[3 * (size_t)i + 2] = dir.z;
	}
	float2 tt = t[i];
	float entry = 0.0f;
	bool miss = false;
	if (!raabb_contains(M, org)) {
		const float e = aabb_ray_entry(M.raabb_min, M.raabb_max, m3_mulv(M.r2l, org), m3_mulv(M.r2l, dir));
		miss = !(e > 0.0f && e < 3.402823466e+38f); // (a box behind the origin has a slab overlap at negative t)
		entry = e + 1e-6f;
	}
	tt.x = miss ? tt.y : fmaxf(tt.x, entry);
	t[i] = tt;
}

// hemisphere rays of ngp_irradiance_rays: ray r = r0 + i of the request is ray k = r % K of point r / K, k = u + n_u v, stratum centre
// (a, b) = ((u + .5) / n_u, (v + .5) / n_v), Malley's cosine-weighted direction local_frame(n) (sqrt(a) cos 2 pi b, sqrt(a) sin 2 pi b,
// sqrt(1 - a)); origin p + offset n; t = (0, the closest triangle hit over all meshes, +inf without one). positions / normals hold the
// points from r0 / K on.
__global__ void irradiance_rays_kernel(const MeshSceneParams S, int occlude, uint32_t n_u, uint32_t n_v, float offset, unsigned long long r0, uint32_t n,
                                       const float* __restrict__ positions, const float* __restrict__ normals, float* __restrict__ o_out,
                                       float* __restrict__ d_out, float2* __restrict__ t_out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const unsigned long long K = (unsigned long long)n_u * n_v, r = r0 + i, pt = r / K, pl = pt - r0 / K;
	const uint32_t k = (uint32_t)(r - pt * K), u = k % n_u, v = k / n_u;
	const f3 nrm = normalize3(ld3(normals + 3 * pl));
	const float a = ((float)u + 0.5f) / (float)n_u, b = ((float)v + 0.5f) / (float)n_v;
	const float sa = sqrtf(a), phi = 2.0f * 3.14159265358979323846f * b;
	float frame[9];
	local_frame(nrm, frame);
	const f3 dir = normalize3(m3_mulv(frame, mk3(sa * cosf(phi), sa * sinf(phi), sqrtf(1.0f - a))));
	const f3 org = add3(ld3(positions + 3 * pl), scale3(nrm, offset));
	const float t_max = occlude ? closest_hit(S, org, dir) : __builtin_huge_valf();
	o_out[3 * (size_t)i] = org.x; o_out[3 * (size_t)i + 1] = org.y; o_out[3 * (size_t)i + 2] = org.z;
	d_out[3 * (size_t)i] = dir.x; d_out[3 * (size_t)i + 1] = dir.y; d_out[3 * (size_t)i + 2] = dir.z;
	t_out[i] = make_float2(0.0f, t_max);
}

// one wave per point: the sum of its rays' rgb among rays [r0, r0 + n) of the request, lane-strided then a butterfly (a fixed order, no
// atomics), and the count of rays no mesh blocks. A point whose rays span several chunks (K > the chunk) adds the chunks' sums in chunk
// order in part[0]; its last chunk writes out = ((pi / K) sum rgb, unblocked / K). out holds the points from r0 / K on.
__global__ void irradiance_reduce_kernel(uint32_t K, unsigned long long r0, uint32_t n, const float4* __restrict__ rgba, const float2* __restrict__ t,
                                         float4* __restrict__ part, float4* __restrict__ out) {
	const unsigned long long pt = r0 / K + (blockIdx.x * blockDim.x + threadIdx.x) / 64u;
	const int lane = threadIdx.x & 63;
	const unsigned long long lo_p = pt * K, hi_p = lo_p + K, r1 = r0 + n;
	if (lo_p >= r1) return; // (wave-uniform)
	const unsigned long long lo = lo_p > r0 ? lo_p : r0, hi = hi_p < r1 ? hi_p : r1;
	float sr = 0.f, sg = 0.f, sb = 0.f;
	uint32_t c = 0;
	for (unsigned long long r = lo + lane; r < hi; r += 64u) {
		const float4 x = rgba[r - r0];
		sr += x.x; sg += x.y; sb += x.z;
		c += t[r - r0].y == __builtin_huge_valf() ? 1u : 0u;
	}
#pragma unroll
	for (int m = 32; m >= 1; m >>= 1) {
		sr += __shfl_xor(sr, m);
		sg += __shfl_xor(sg, m);
		sb += __shfl_xor(sb, m);
		c += __shfl_xor(c, m);
	}
	if (lane != 0) return;
	if (lo != lo_p) { // not the point's first chunk
		const float4 p = part[0];
		sr = p.x + sr; sg = p.y + sg; sb = p.z + sb; c += __float_as_uint(p.w);
	}
	if (hi == hi_p) {
		const float scale = 3.14159265358979323846f / (float)K;
		out[pt - r0 / K] = make_float4(sr * scale, sg * scale, sb * scale, (float)((double)c / (double)K));
	} else {
		part[0] = make_float4(sr, sg, sb, __uint_as_float(c));
	}
}

void launch_ray_list_prep(const ModelParams& M, uint32_t n, const float* o, float* d, float2* t, bool normalize, hipStream_t stream) {
	if (n) hipLaunchKernelGGL(ray_list_prep_kernel, dim3((n + 127) / 128), dim3(128), 0, stream, M, n, o, d, t, normalize ? 1 : 0);
}
void launch_irradiance_rays(const MeshSceneParams& S, bool occlude, uint32_t n_u, uint32_t n_v, float offset, uint64_t r0, uint32_t n, const float* positions,
                            const float* normals, float* o, float* d, float2* t, hipStream_t stream) {
	if (n) hipLaunchKernelGGL(irradiance_rays_kernel, dim3((n + 127) / 128), dim3(128), 0, stream, S, occlude ? 1 : 0, n_u, n_v, offset, (unsigned long long)r0, n,
	                          positions, normals, o, d, t);
}
void launch_irradiance_reduce(uint32_t K, uint64_t r0, uint32_t n, const float4* rgba, const float2* t, float4* part, float4* out, hipStream_t stream) {
	if (!n) return;
	const uint64_t n_pts = (r0 + n - 1) / K - r0 / K + 1; // points the chunk touches
	hipLaunchKernelGGL(irradiance_reduce_kernel, dim3((unsigned)((n_pts + 3) / 4)), dim3(256), 0, stream, K, (unsigned long long)r0, n, rgba, t, part, out);
}


// ---- SH9 irradiance volumes (ngp_irradiance_sphere_rays, ngp_irradiance_sh_traced, ngp_irradiance_volume_at; contract in
// include/ngp_hip.h, basis in sh9.h). One sphere of rays per probe through the ray-list tracer, projected onto nine coefficients per
// channel; a lookup blends the up to 8 probes around a point and evaluates the clamped-cosine convolution at the normal.

// direction k = u + n_u v of the sphere, the same for every probe: the centre of an equal-area stratum, z = 1 - 2 a, phi = 2 pi b with
// (a, b) = ((u + .5) / n_u, (v + .5) / n_v). sqrt(1 - z^2) is formed as 2 sqrt(a (1 - a)), which loses nothing near the poles, and the
// azimuth's sine and cosine from 2 b in half turns (no rounded 2 pi b). The generator and the reduction both call this.
NGP_DEV f3 sphere_dir(uint32_t k, uint32_t n_u, uint32_t n_v) {
	const uint32_t u = k % n_u, v = k / n_u;
	const float a = ((float)u + 0.5f) / (float)n_u, b = ((float)v + 0.5f) / (float)n_v;
	const float s = 2.0f * sqrtf(a * (1.0f - a));
	float sn, cs;
	sincospif(2.0f * b, &sn, &cs);
	return normalize3(mk3(s * cs, s * sn, 1.0f - 2.0f * a));
}

// the n rays of a chunk of whole probes: ray i is direction i % K of the chunk's probe i / K; origin = the probe's position, t = (0, the
// closest triangle hit over all meshes as in irradiance_rays_kernel, +inf without one). positions holds the chunk's probes.
__global__ void irradiance_sphere_rays_kernel(const MeshSceneParams S, int occlude, uint32_t n_u, uint32_t n_v, uint32_t n, const float* __restrict__ positions,
                                              float* __restrict__ o_out, float* __restrict__ d_out, float2* __restrict__ t_out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t K = n_u * n_v, pl = i / K, k = i - pl * K;
	const f3 dir = sphere_dir(k, n_u, n_v);
	const f3 org = ld3(positions + 3 * (size_t)pl);
	const float t_max = occlude ? closest_hit(S, org, dir) : __builtin_huge_valf();
	o_out[3 * (size_t)i] = org.x; o_out[3 * (size_t)i + 1] = org.y; o_out[3 * (size_t)i + 2] = org.z;
	d_out[3 * (size_t)i] = dir.x; d_out[3 * (size_t)i + 1] = dir.y; d_out[3 * (size_t)i + 2] = dir.z;
	t_out[i] = make_float2(0.0f, t_max);
}

// one wave per probe, four per workgroup: c[3 m + ch] = (4 pi / K) sum_k L_ch(w_k) Y_m(w_k) over the probe's K rays (rgba, t: the chunk's
// rays, probe p's at p K on), lane-strided with w_k recomputed from k (no direction array is read: 24 B a ray), then a butterfly in a fixed
// order; no atomics, so a probe's record does not depend on the run or on which other probes the launch carries. Lane 0 writes the
// record: 27 coefficients and w = unblocked / K, as 7 float4 at out[7 p].
__global__ void irradiance_sh_reduce_kernel(uint32_t n_u, uint32_t n_v, uint32_t n_probes, const float4* __restrict__ rgba, const float2* __restrict__ t,
                                            float4* __restrict__ out) {
	const uint32_t p = (blockIdx.x * blockDim.x + threadIdx.x) / 64u;
	if (p >= n_probes) return; // (wave-uniform)
	const uint32_t lane = threadIdx.x & 63u, K = n_u * n_v;
	const size_t base = (size_t)p * K;
	float acc[27];
#pragma unroll
	for (int j = 0; j < 27; ++j) acc[j] = 0.f;
	uint32_t c = 0;
	for (uint32_t k = lane; k < K; k += 64u) {
		const float4 L = rgba[base + k];
		const f3 w = sphere_dir(k, n_u, n_v);
		float Y[9];
		sh9_basis(w.x, w.y, w.z, Y);
#pragma unroll
		for (int m = 0; m < 9; ++m) {
			acc[3 * m] += L.x * Y[m];
			acc[3 * m + 1] += L.y * Y[m];
			acc[3 * m + 2] += L.z * Y[m];
		}
		c += t[base + k].y == __builtin_huge_valf() ? 1u : 0u;
	}
#pragma unroll
	for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
		for (int j = 0; j < 27; ++j) acc[j] += __shfl_xor(acc[j], s);
		c += __shfl_xor(c, s);
	}
	if (lane != 0) return;
	const float scale = 4.0f * 3.14159265358979323846f / (float)K;
#pragma unroll
	for (int j = 0; j < 27; ++j) acc[j] *= scale;
	float4* o = out + 7 * (size_t)p;
#pragma unroll
	for (int q = 0; q < 6; ++q) o[q] = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
	o[6] = make_float4(acc[24], acc[25], acc[26], (float)((double)c / (double)K));
}

// one thread per point: out = (E rgb, W) of irradiance_volume_lookup at the point and its normalised normal
__global__ void irradiance_volume_lookup_kernel(const IrradianceVolume V, uint32_t n, const float* __restrict__ positions, const float* __restrict__ normals,
                                                float4* __restrict__ out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	float E[3], W;
	irradiance_volume_lookup(V, ld3(positions + 3 * (size_t)i), normalize3(ld3(normals + 3 * (size_t)i)), E, W);
	out[i] = make_float4(E[0], E[1], E[2], W);
}

// one wave per probe, four per workgroup: lane q owns texel q of the probe's distance map and sums rho = max(0, w_q . w_k)^(2^e), rho d and
// rho d^2 over the probe's K rays in k order, d = min(t_max, D) (t: the chunk's rays as irradiance_sphere_rays_kernel wrote them, probe p's
// at p K on). The rays are staged 64 at a time: lane j forms (w_k, d_k) of ray 64 c + j once and puts it into the wave's 1 KB of LDS, then
// every lane walks the staged rays (all lanes read one address: a broadcast). No atomics and no butterfly: a map does not depend on the
// run or on which other probes the launch carries. Every wave of a workgroup runs the same number of barriers (K is the launch's); a wave
// past the last probe works on the last probe again and stores nothing.
__global__ void __launch_bounds__(256) irradiance_distance_reduce_kernel(uint32_t n_u, uint32_t n_v, uint32_t n_probes, uint32_t sharpness_log2, float D,
                                                                         const float2* __restrict__ t, float2* __restrict__ out) {
	__shared__ float4 staged[4][64];
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, K = n_u * n_v;
	const uint32_t p_own = blockIdx.x * 4u + wave;
	const bool live = p_own < n_probes;
	const uint32_t p = live ? p_own : n_probes - 1u;
	const size_t base = (size_t)p * K;
	const f3 wq = distance_texel_dir(lane);
	float S = 0.f, s1 = 0.f, s2 = 0.f;
	for (uint32_t k0 = 0; k0 < K; k0 += 64u) {
		const uint32_t k = k0 + lane;
		float4 ray = make_float4(0.f, 0.f, 0.f, 0.f);
		if (k < K) { // (a tail chunk: no read past the probe's rays)
			const f3 w = sphere_dir(k, n_u, n_v);
			ray = make_float4(w.x, w.y, w.z, fminf(t[base + k].y, D));
		}
		staged[wave][lane] = ray;
		__syncthreads();
		const uint32_t m = K - k0 < 64u ? K - k0 : 64u; // (and no weight for a missing ray)
		for (uint32_t j = 0; j < m; ++j) {
			const float4 r = staged[wave][j];
			float rho = fmaxf(0.0f, (wq.x * r.x + wq.y * r.y) + wq.z * r.z);
			for (uint32_t i = 0; i < sharpness_log2; ++i) rho *= rho;
			const float rd = rho * r.w;
			S += rho;
			s1 += rd;
			s2 += rd * r.w;
		}
		__syncthreads(); // the next chunk overwrites the stage
	}
	if (!live) return; // (behind the last barrier)
	out[(size_t)p * DISTANCE_MAP_TEXELS + lane] = S > 0.0f ? make_float2(s1 / S, s2 / S) : make_float2(D, D * D);
}

// one thread per point: out = (E rgb, W') of irradiance_volume_lookup_visible at the point and its normalised normal
__global__ void irradiance_volume_lookup_visible_kernel(const IrradianceVolumeVisible A, uint32_t n, const float* __restrict__ positions, const float* __restrict__ normals,
                                                        float4* __restrict__ out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	float E[3], W;
	irradiance_volume_lookup_visible(A, ld3(positions + 3 * (size_t)i), normalize3(ld3(normals + 3 * (size_t)i)), E, W);
	out[i] = make_float4(E[0], E[1], E[2], W);
}

void launch_irradiance_distance_reduce(uint32_t n_u, uint32_t n_v, uint32_t n_probes, uint32_t sharpness_log2, float D, const float2* t, float2* out, hipStream_t stream) {
	if (n_probes) hipLaunchKernelGGL(irradiance_distance_reduce_kernel, dim3((n_probes + 3) / 4), dim3(256), 0, stream, n_u, n_v, n_probes, sharpness_log2, D, t, out);
}
void launch_irradiance_volume_lookup_visible(const IrradianceVolumeVisible& A, uint32_t n, const float* positions, const float* normals, float4* out, hipStream_t stream) {
	if (n) hipLaunchKernelGGL(irradiance_volume_lookup_visible_kernel, dim3((n + 127) / 128), dim3(128), 0, stream, A, n, positions, normals, out);
}
void launch_irradiance_sphere_rays(const MeshSceneParams& S, bool occlude, uint32_t n_u, uint32_t n_v, uint32_t n, const float* positions, float* o, float* d, float2* t,
                                   hipStream_t stream) {
	if (n) hipLaunchKernelGGL(irradiance_sphere_rays_kernel, dim3((n + 127) / 128), dim3(128), 0, stream, S, occlude ? 1 : 0, n_u, n_v, n, positions, o, d, t);
}
void launch_irradiance_sh_reduce(uint32_t n_u, uint32_t n_v, uint32_t n_probes, const float4* rgba, const float2* t, float4* out, hipStream_t stream) {
	if (n_probes) hipLaunchKernelGGL(irradiance_sh_reduce_kernel, dim3((n_probes + 3) / 4), dim3(256), 0, stream, n_u, n_v, n_probes, rgba, t, out);
}
void launch_irradiance_volume_lookup(const IrradianceVolume& V, uint32_t n, const float* positions, const float* normals, float4* out, hipStream_t stream) {
	if (n) hipLaunchKernelGGL(irradiance_volume_lookup_kernel, dim3((n + 127) / 128), dim3(128), 0, stream, V, n, positions, normals, out);
}


// ---- diffuse interreflection (ngp_compute_irradiance_volume_bounced, ngp_irradiance_sh_bounce; contract in include/ngp_hip.h, "bounces").
// One pass feeds a volume back into itself at the mesh hits of its probes' sphere rays: the rays of irradiance_sphere_rays_kernel, the
// closest hit with its mesh and triangle kept, the volume's estimate at the hit, and irradiance_sh_reduce_kernel unchanged behind it.

// the n rays of a chunk of whole probes, one thread a ray: rgba_out = (B rgb, t of the hit or +inf), t_out = (0, the same t) as the
// projection counts it. B = (1 - alpha) albedo max(E, 0) / pi with (E, W) the lookup A at the hit point o + t w and the hit triangle's
// winding normal turned against the ray; 0 without a hit and where W = 0. alpha: the chunk's rays' NeRF alpha (nullptr: 0). The lookup's
// accumulators are live behind the traversals only, as in render_mesh_fused.
// where a hit's albedo (a bounce pass) or its sun source (a sun pass) comes from: the call's three scalars for every mesh, or one float4 of
// the call's table of one entry a mesh (ngp_hip.h, "mesh albedos"). The table's entry is read where the values are first used, behind the
// traversals: one 16-byte load a hit ray.
struct CallColour {
	f3 v;
	NGP_DEV f3 operator()(int) const { return v; }
};
struct MeshColour {
	const float4* __restrict__ table;
	NGP_DEV f3 operator()(int mesh) const {
		const float4 c = table[mesh];
		return mk3(c.x, c.y, c.z);
	}
};

// ray i of a chunk of whole probes in a bounce pass: B as the kernels below state it, albedo(mesh) the hit mesh's; returns t of the hit.
// A by reference: by value the visible kernel's prologue came out in another order.
template <typename Lookup, typename Albedo>
NGP_DEV float bounce_ray(const MeshSceneParams S, const Lookup& A, int occlude, uint32_t n_u, uint32_t n_v, uint32_t i, const float* __restrict__ positions, const Albedo albedo,
                         const float* __restrict__ alpha, f3& B) {
	const uint32_t K = n_u * n_v, pl = i / K, k = i - pl * K;
	const f3 dir = sphere_dir(k, n_u, n_v);
	const f3 org = ld3(positions + 3 * (size_t)pl);
	int mesh = -1, tri_idx = -1;
	const float t_max = occlude ? closest_hit(S, org, dir, &mesh, &tri_idx) : __builtin_huge_valf();
	B = mk3(0.f, 0.f, 0.f);
	if (mesh > -1) {
		const Triangle& tri = S.meshes[mesh].tris[tri_idx];
		const f3 a = ld3(tri.a);
		const f3 N = normalize3(cross3(sub3(ld3(tri.b), a), sub3(ld3(tri.c), a)));
		const f3 nff = dot3(N, dir) < 0.0f ? N : scale3(N, -1.0f);
		const f3 h = add3(org, scale3(dir, t_max));
		float E[3], W;
		if constexpr (std::is_same<Lookup, IrradianceVolumeVisible>::value) irradiance_volume_lookup_visible(A, h, nff, E, W);
		else irradiance_volume_lookup(A, h, nff, E, W);
		if (W > 0.0f) {
			const float through = 1.0f - (alpha ? alpha[i] : 0.0f);
			const f3 al = albedo(mesh);
			B = mk3(through * (al.x * fmaxf(E[0], 0.0f) / PI_F), through * (al.y * fmaxf(E[1], 0.0f) / PI_F), through * (al.z * fmaxf(E[2], 0.0f) / PI_F));
		}
	}
	return t_max;
}

template <typename Lookup>
__global__ void irradiance_bounce_rays_kernel(const MeshSceneParams S, const Lookup A, int occlude, uint32_t n_u, uint32_t n_v, uint32_t n, const float* __restrict__ positions,
                                              float albedo_r, float albedo_g, float albedo_b, const float* __restrict__ alpha, float4* __restrict__ rgba_out,
                                              float2* __restrict__ t_out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	f3 B;
	const float t_max = bounce_ray(S, A, occlude, n_u, n_v, i, positions, CallColour{mk3(albedo_r, albedo_g, albedo_b)}, alpha, B);
	rgba_out[i] = make_float4(B.x, B.y, B.z, t_max);
	t_out[i] = make_float2(0.0f, t_max);
}
// the same pass with every mesh's own albedo: albedos[m] = (a_m rgb, unused), resolved by the host for the call (ngp_hip.h, "mesh albedos")
template <typename Lookup>
__global__ void irradiance_bounce_rays_mesh_albedo_kernel(const MeshSceneParams S, const Lookup A, int occlude, uint32_t n_u, uint32_t n_v, uint32_t n,
                                                          const float* __restrict__ positions, const float4* __restrict__ albedos, const float* __restrict__ alpha,
                                                          float4* __restrict__ rgba_out, float2* __restrict__ t_out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	f3 B;
	const float t_max = bounce_ray(S, A, occlude, n_u, n_v, i, positions, MeshColour{albedos}, alpha, B);
	rgba_out[i] = make_float4(B.x, B.y, B.z, t_max);
	t_out[i] = make_float2(0.0f, t_max);
}

// out = v0 + r on the 27 coefficients of every record, one thread per float4 (7 a probe); the seventh keeps v0's w
__global__ void irradiance_volume_add_kernel(uint32_t n_float4, const float4* __restrict__ v0, const float4* __restrict__ r, float4* __restrict__ out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_float4) return;
	const float4 a = v0[i], b = r[i];
	out[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, i % 7u == 6u ? a.w : a.w + b.w);
}

// alpha[i] = rgba[i].w: the tracer's alpha of a chunk's rays, kept for the bounce passes
__global__ void ray_alpha_kernel(uint32_t n, const float4* __restrict__ rgba, float* __restrict__ alpha) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) alpha[i] = rgba[i].w;
}

// VV != nullptr: the lookup weighted by the probes' visibility, and V is not looked at. albedos != nullptr: the device table of one
// float4 a mesh, and albedo is not looked at
void launch_irradiance_bounce_rays(const MeshSceneParams& S, const IrradianceVolume& V, const IrradianceVolumeVisible* VV, bool occlude, uint32_t n_u, uint32_t n_v, uint32_t n,
                                   const float* positions, const float* albedo, const float4* albedos, const float* alpha, float4* rgba, float2* t, hipStream_t stream) {
	if (!n) return;
	const dim3 blocks((n + 127) / 128), threads(128);
	if (albedos) {
		if (VV) hipLaunchKernelGGL(irradiance_bounce_rays_mesh_albedo_kernel<IrradianceVolumeVisible>, blocks, threads, 0, stream, S, *VV, occlude ? 1 : 0, n_u, n_v, n, positions, albedos, alpha, rgba, t);
		else hipLaunchKernelGGL(irradiance_bounce_rays_mesh_albedo_kernel<IrradianceVolume>, blocks, threads, 0, stream, S, V, occlude ? 1 : 0, n_u, n_v, n, positions, albedos, alpha, rgba, t);
		return;
	}
	if (VV) hipLaunchKernelGGL(irradiance_bounce_rays_kernel<IrradianceVolumeVisible>, blocks, threads, 0, stream, S, *VV, occlude ? 1 : 0, n_u, n_v, n, positions, albedo[0], albedo[1], albedo[2], alpha, rgba, t);
	else hipLaunchKernelGGL(irradiance_bounce_rays_kernel<IrradianceVolume>, blocks, threads, 0, stream, S, V, occlude ? 1 : 0, n_u, n_v, n, positions, albedo[0], albedo[1], albedo[2], alpha, rgba, t);
}
void launch_irradiance_volume_add(uint32_t n_float4, const float4* v0, const float4* r, float4* out, hipStream_t stream) {
	if (n_float4) hipLaunchKernelGGL(irradiance_volume_add_kernel, dim3((n_float4 + 255) / 256), dim3(256), 0, stream, n_float4, v0, r, out);
}
void launch_ray_alpha(uint32_t n, const float4* rgba, float* alpha, hipStream_t stream) {
	if (n) hipLaunchKernelGGL(ray_alpha_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, rgba, alpha);
}


// ---- sun light on the meshes as a bounce source (ngp_compute_irradiance_volume_sunlit, ngp_irradiance_sh_sun; contract in
// include/ngp_hip.h, "sun"). One pass puts the sun's first bounce off the meshes into the records: the rays of
// irradiance_sphere_rays_kernel, the closest hit with its mesh and triangle kept, a shadow query from the hit towards the sun, and
// irradiance_sh_reduce_kernel unchanged behind it.

#ifdef NGP_EXPERIMENT_SUN_ANY_HIT // tools/irradiance_bounce_rate.py --sun alone: the shadow query as an any-hit traversal. Measured against the closest hit it buys 4-6 % of a sun pass, inside the spread of repeats, so it does not ship.
// is any triangle of one mesh hit at 0 <= t < MAX_DIST? The traversal of bvh4_ray_intersect without what only the closest hit needs: the
// children are not sorted, the range never shrinks (every child whose box entry lies below MAX_DIST is pushed), and the first triangle
// inside the range ends the walk.
NGP_DEV bool bvh4_ray_occluded(const TriangleBvhNode* __restrict__ nodes, const Triangle* __restrict__ tris, f3 ro, f3 rd) {
	int stack[BVH4_STACK_SIZE];
	int sp = 0;
	stack[sp++] = 0;
	while (sp > 0) {
		int idx = stack[--sp];
		const int left = nodes[idx].left_idx, right = nodes[idx].right_idx;
		if (left < 0) {
			int end = -right - 1;
			for (int i = -left - 1; i < end; ++i) {
				if (tri_ray_intersect(tris[i], ro, rd) < MAX_DIST) return true;
			}
		} else {
#pragma unroll
			for (uint32_t i = 0; i < 4; ++i) {
				const TriangleBvhNode& c = nodes[left + (int)i];
				if (aabb_ray_entry(c.bmin, c.bmax, ro, rd) < MAX_DIST && sp < BVH4_STACK_SIZE) stack[sp++] = left + (int)i;
			}
		}
	}
	return false;
}
#endif

// is the ray blocked by a triangle of any mesh within MAX_DIST? The closest hit decides: it finds every hit inside the traversal's range.
// S by value, as in closest_hit.
NGP_DEV bool any_hit(const MeshSceneParams S, f3 org, f3 dir) {
#ifdef NGP_EXPERIMENT_SUN_ANY_HIT
	for (uint32_t m = 0; m < S.n_meshes; ++m)
		if (bvh4_ray_occluded(S.meshes[m].nodes, S.meshes[m].tris, org, dir)) return true;
	return false;
#else
	return closest_hit(S, org, dir) < MAX_DIST;
#endif
}

// ray i of a chunk of whole probes under the sun: B_ch = (1 - alpha) albedo_ch radiance_ch c vis / pi with c = N_ff . sun (N_ff the hit
// triangle's winding normal turned against the ray, sun a unit vector), vis = 0 where a triangle of any mesh lies within MAX_DIST of
// q = h + bias N_ff along sun; 0 without a hit and where c <= 0. Returns t of the primary hit (+inf without one). alpha: the chunk's rays'
// NeRF alpha (nullptr: 0). No volume is read. lit: the ray has a hit, c > 0 and vis = 1, and q is that ray's lifted hit point (zeros
// otherwise); a caller that drops both keeps the code it had before they were returned. S by value, as in closest_hit.
// source(mesh): albedo x radiance of the hit's mesh (CallColour: one for all; MeshColour: the call's table).
template <typename Source>
NGP_DEV float sun_ray(const MeshSceneParams S, int occlude, uint32_t n_u, uint32_t n_v, uint32_t i, const float* __restrict__ positions, f3 sun, float bias, const Source source_of,
                      const float* __restrict__ alpha, f3& B, f3& q_out, bool& lit) {
	const uint32_t K = n_u * n_v, pl = i / K, k = i - pl * K;
	const f3 dir = sphere_dir(k, n_u, n_v);
	const f3 org = ld3(positions + 3 * (size_t)pl);
	int mesh = -1, tri_idx = -1;
	const float t_max = occlude ? closest_hit(S, org, dir, &mesh, &tri_idx) : __builtin_huge_valf();
	B = mk3(0.f, 0.f, 0.f);
	q_out = mk3(0.f, 0.f, 0.f);
	lit = false;
	if (mesh > -1) {
		const Triangle& tri = S.meshes[mesh].tris[tri_idx];
		const f3 a = ld3(tri.a);
		const f3 N = normalize3(cross3(sub3(ld3(tri.b), a), sub3(ld3(tri.c), a)));
		const f3 nff = dot3(N, dir) < 0.0f ? N : scale3(N, -1.0f);
		const float c = dot3(nff, sun);
		if (c > 0.0f) {
			const f3 h = add3(org, scale3(dir, t_max));
			const f3 q = add3(h, scale3(nff, bias));
			if (!any_hit(S, q, sun)) {
				const float through = 1.0f - (alpha ? alpha[i] : 0.0f);
				const f3 source = source_of(mesh);
				B = mk3(through * (source.x * c / PI_F), through * (source.y * c / PI_F), through * (source.z * c / PI_F));
				q_out = q;
				lit = true;
			}
		}
	}
	return t_max;
}

// the n rays of a chunk of whole probes, one thread a ray: rgba_out = (B rgb, t of the hit or +inf), t_out = (0, the same t) as the
// projection counts it; B as sun_ray forms it.
__global__ void irradiance_sun_rays_kernel(const MeshSceneParams S, int occlude, uint32_t n_u, uint32_t n_v, uint32_t n, const float* __restrict__ positions, float sun_x,
                                           float sun_y, float sun_z, float bias, float source_r, float source_g, float source_b, const float* __restrict__ alpha,
                                           float4* __restrict__ rgba_out, float2* __restrict__ t_out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	f3 B, q;
	bool lit;
	const float t_max = sun_ray(S, occlude, n_u, n_v, i, positions, mk3(sun_x, sun_y, sun_z), bias, CallColour{mk3(source_r, source_g, source_b)}, alpha, B, q, lit);
	rgba_out[i] = make_float4(B.x, B.y, B.z, t_max);
	t_out[i] = make_float2(0.0f, t_max);
}

// the same pass with every mesh's own source: sources[m] = (fl(a_m radiance) rgb, unused), formed by the host for the call
__global__ void irradiance_sun_rays_mesh_albedo_kernel(const MeshSceneParams S, int occlude, uint32_t n_u, uint32_t n_v, uint32_t n, const float* __restrict__ positions,
                                                       float sun_x, float sun_y, float sun_z, float bias, const float4* __restrict__ sources, const float* __restrict__ alpha,
                                                       float4* __restrict__ rgba_out, float2* __restrict__ t_out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	f3 B, q;
	bool lit;
	const float t_max = sun_ray(S, occlude, n_u, n_v, i, positions, mk3(sun_x, sun_y, sun_z), bias, MeshColour{sources}, alpha, B, q, lit);
	rgba_out[i] = make_float4(B.x, B.y, B.z, t_max);
	t_out[i] = make_float2(0.0f, t_max);
}

// ---- the NeRF's density in front of the sun (ngp_compute_irradiance_volume_sunlit_shadowed, ngp_irradiance_sh_sun_shadowed; contract in
// include/ngp_hip.h, "sun"). The generator below also writes the chunk's shadow-ray list for the ray-list tracer, one entry per probe ray
// in the chunk's own layout (no compaction: any chunking gives the same bytes); the apply kernel scales B by what the tracer let through.

// irradiance_sun_rays_kernel, and entry i of the shadow-ray list: origin q, direction sun, t = (t_min, +inf) for a ray the sun lights;
// origin 0, t = (0, 0) for every other ray, which ray_list_prep_kernel leaves dead
__global__ void irradiance_sun_shadow_rays_kernel(const MeshSceneParams S, int occlude, uint32_t n_u, uint32_t n_v, uint32_t n, const float* __restrict__ positions, float sun_x,
                                                  float sun_y, float sun_z, float bias, float source_r, float source_g, float source_b, const float* __restrict__ alpha,
                                                  float t_min, float4* __restrict__ rgba_out, float2* __restrict__ t_out, float* __restrict__ o_out, float* __restrict__ d_out,
                                                  float2* __restrict__ st_out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	f3 B, q;
	bool lit;
	const float t_max = sun_ray(S, occlude, n_u, n_v, i, positions, mk3(sun_x, sun_y, sun_z), bias, CallColour{mk3(source_r, source_g, source_b)}, alpha, B, q, lit);
	rgba_out[i] = make_float4(B.x, B.y, B.z, t_max);
	t_out[i] = make_float2(0.0f, t_max);
	o_out[3 * (size_t)i] = q.x; o_out[3 * (size_t)i + 1] = q.y; o_out[3 * (size_t)i + 2] = q.z;
	d_out[3 * (size_t)i] = sun_x; d_out[3 * (size_t)i + 1] = sun_y; d_out[3 * (size_t)i + 2] = sun_z;
	st_out[i] = lit ? make_float2(t_min, __builtin_huge_valf()) : make_float2(0.0f, 0.0f);
}

// the same generator with every mesh's own source (irradiance_sun_rays_mesh_albedo_kernel's table)
__global__ void irradiance_sun_shadow_rays_mesh_albedo_kernel(const MeshSceneParams S, int occlude, uint32_t n_u, uint32_t n_v, uint32_t n, const float* __restrict__ positions,
                                                              float sun_x, float sun_y, float sun_z, float bias, const float4* __restrict__ sources,
                                                              const float* __restrict__ alpha, float t_min, float4* __restrict__ rgba_out, float2* __restrict__ t_out,
                                                              float* __restrict__ o_out, float* __restrict__ d_out, float2* __restrict__ st_out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	f3 B, q;
	bool lit;
	const float t_max = sun_ray(S, occlude, n_u, n_v, i, positions, mk3(sun_x, sun_y, sun_z), bias, MeshColour{sources}, alpha, B, q, lit);
	rgba_out[i] = make_float4(B.x, B.y, B.z, t_max);
	t_out[i] = make_float2(0.0f, t_max);
	o_out[3 * (size_t)i] = q.x; o_out[3 * (size_t)i + 1] = q.y; o_out[3 * (size_t)i + 2] = q.z;
	d_out[3 * (size_t)i] = sun_x; d_out[3 * (size_t)i + 1] = sun_y; d_out[3 * (size_t)i + 2] = sun_z;
	st_out[i] = lit ? make_float2(t_min, __builtin_huge_valf()) : make_float2(0.0f, 0.0f);
}

// B' = max(1 - alpha_s, 0) B on the chunk's rays, one float32 product a channel: alpha_s = the tracer's alpha of the ray's shadow ray
// (traced: its rgba), 0 for a ray without one (st.y = 0, as the generator left it; the prep step moves st.x alone). rgba: (B rgb, t) in
// place, t untouched; shadow_out (nullable): (q, alpha_s), zeros without a shadow ray.
__global__ void irradiance_sun_shadow_apply_kernel(uint32_t n, const float4* __restrict__ traced, const float* __restrict__ o, const float2* __restrict__ st,
                                                   float4* __restrict__ rgba, float4* __restrict__ shadow_out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const bool has = st[i].y != 0.0f;
	const float alpha_s = has ? traced[i].w : 0.0f;
	if (has) {
		const float through = fmaxf(1.0f - alpha_s, 0.0f);
		float4 b = rgba[i];
		b.x = through * b.x; b.y = through * b.y; b.z = through * b.z;
		rgba[i] = b;
	}
	if (shadow_out) shadow_out[i] = has ? make_float4(o[3 * (size_t)i], o[3 * (size_t)i + 1], o[3 * (size_t)i + 2], alpha_s) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// sun: the unit direction towards the sun; source: albedo x radiance per channel, as the host forms it in float. sources != nullptr: the
// device table of one float4 a mesh, and source is not looked at
void launch_irradiance_sun_rays(const MeshSceneParams& S, bool occlude, uint32_t n_u, uint32_t n_v, uint32_t n, const float* positions, const float* sun, float bias,
                                const float* source, const float4* sources, const float* alpha, float4* rgba, float2* t, hipStream_t stream) {
	if (!n) return;
	const dim3 blocks((n + 127) / 128), threads(128);
	if (sources) hipLaunchKernelGGL(irradiance_sun_rays_mesh_albedo_kernel, blocks, threads, 0, stream, S, occlude ? 1 : 0, n_u, n_v, n, positions, sun[0], sun[1], sun[2], bias, sources, alpha, rgba, t);
	else hipLaunchKernelGGL(irradiance_sun_rays_kernel, blocks, threads, 0, stream, S, occlude ? 1 : 0, n_u, n_v, n, positions, sun[0], sun[1], sun[2], bias,
	                        source[0], source[1], source[2], alpha, rgba, t);
}
// the same pass with the shadow-ray list of its chunk: o, d (3 n floats each) and st (n) for launch_ray_list_prep and the ray-list tracer
void launch_irradiance_sun_shadow_rays(const MeshSceneParams& S, bool occlude, uint32_t n_u, uint32_t n_v, uint32_t n, const float* positions, const float* sun, float bias,
                                       const float* source, const float4* sources, const float* alpha, float t_min, float4* rgba, float2* t, float* o, float* d, float2* st,
                                       hipStream_t stream) {
	if (!n) return;
	const dim3 blocks((n + 127) / 128), threads(128);
	if (sources) hipLaunchKernelGGL(irradiance_sun_shadow_rays_mesh_albedo_kernel, blocks, threads, 0, stream, S, occlude ? 1 : 0, n_u, n_v, n, positions, sun[0], sun[1], sun[2], bias, sources, alpha,
	                                t_min, rgba, t, o, d, st);
	else hipLaunchKernelGGL(irradiance_sun_shadow_rays_kernel, blocks, threads, 0, stream, S, occlude ? 1 : 0, n_u, n_v, n, positions, sun[0], sun[1], sun[2],
	                        bias, source[0], source[1], source[2], alpha, t_min, rgba, t, o, d, st);
}
void launch_irradiance_sun_shadow_apply(uint32_t n, const float4* traced, const float* o, const float2* st, float4* rgba, float4* shadow_out, hipStream_t stream) {
	if (n) hipLaunchKernelGGL(irradiance_sun_shadow_apply_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, traced, o, st, rgba, shadow_out);
}

// ---- the meshes in front of the sun on the NeRF (ngp_set_mesh_shadow_on_nerf; contract in include/ngp_hip.h, "sun: the meshes in front of
// the sun on the NeRF"). The frame's NeRF launch composited over zeros into `nerf` instead of the frame: nerf[idx] = the pixel's premultiplied
// (r, g, b, a), zero bits where the launch wrote nothing. This kernel finishes shade_ray's composite over the mesh pass's frame_buffer[idx],
// in shade_ray's order, with the NeRF's colour scaled by f where a mesh stands between the pixel's surface point and the sun. A pixel of
// alpha > 0.2 owns depth_buffer[idx] (shade_ray's rule), so its surface point lies at that z-depth on the ray init_ray forms for it.
// record: (p, 2 blocked / 1 open), left as the host cleared it where the pixel owns no surface point.
// shade_ray's composite of the NeRF's premultiplied n, its colour scaled by f, over the mesh pass's pixel fb, in shade_ray's order
NGP_DEV float4 nerf_over_mesh(float4 fb, float4 n, float f) {
	const float r = n.x * f, g = n.y * f, b = n.z * f, a = n.w;
	float k = 1.0f - a;
	fb.x = r + fb.x * k;
	fb.y = g + fb.y * k;
	fb.z = b + fb.z * k;
	fb.w = a + fb.w * k;
	return fb;
}
__global__ void nerf_mesh_shadow_kernel(const MeshSceneParams S, const MeshShadeParams P, const ModelParams M, const CameraParams C, float4* __restrict__ frame_buffer,
                                        const float* __restrict__ depth_buffer, const float4* __restrict__ nerf, float4* __restrict__ record, const FrameLayout L,
                                        float strength, float bias) {
	uint32_t x, y, idx;
	if (!frame_pixel(L, C, x, y, idx)) return;
	const float4 n = nerf[idx];
	if (n.w == 0.0f) return; // the NeRF pass wrote nothing here: the pixel stays the mesh pass's
	float f = 1.0f;
	if (n.w > 0.2f) {
		const f3 p = nerf_surface_point(M, C, x, y, depth_buffer[idx]); // (render_common.h: the one definition of p)
		const f3 sdir = shadow_ray_dir(P);
		const bool blocked = any_hit(S, add3(p, scale3(sdir, bias)), sdir);
		if (blocked) f = 1.0f - strength;
		record[idx] = make_float4(p.x, p.y, p.z, blocked ? 2.0f : 1.0f);
	}
	frame_buffer[idx] = nerf_over_mesh(frame_buffer[idx], n, f);
}

void launch_nerf_mesh_shadow(const MeshSceneParams& S, const MeshShadeParams& P, const ModelParams& M, const CameraParams& C, float4* frame_buffer, const float* depth_buffer,
                             const float4* nerf, float4* record, const FrameLayout& L, float strength, float bias, hipStream_t stream) {
	hipLaunchKernelGGL(nerf_mesh_shadow_kernel, pixel_blocks(C), pixel_threads(), 0, stream, S, P, M, C, frame_buffer, depth_buffer, nerf, record, L, strength, bias);
}

// ---- the sun's disk (ngp_set_sun_disk; contract in include/ngp_hip.h, "sun: the sun's disk"). K shadow rays a pixel along the sample's
// table D, each tested against ALL meshes (any_hit); the blocked count replaces the boolean on mesh pixels (mesh_sun_disk_kernel, between
// mesh_gbuffer_kernel and the shadow list's prep step) and on NeRF pixels (nerf_mesh_soft_shadow_kernel, in nerf_mesh_shadow_kernel's place).

// the lane of the n-th set bit of m (n < popcount(m)): a select by halves
NGP_DEV uint32_t nth_set_lane(unsigned long long m, uint32_t n) {
	uint32_t pos = 0;
#pragma unroll
	for (uint32_t w = 32; w >= 1; w >>= 1) {
		const uint32_t c = (uint32_t)__popcll((m >> pos) & ((1ull << w) - 1ull));
		if (n >= c) {
			n -= c;
			pos += w;
		}
	}
	return pos;
}

// count = the number of k < K with any_hit(S, q, d_k), for every lane with owner set; 0 for the others. The one definition of the count:
// both kernels call it, with every lane of the wave alive (it ballots and shuffles).
// WAVE: the wave ballots its owners and deals (owner, k) items over its lanes, K adjacent lanes to a pixel, in rounds of 64 / K owners. The
// K rays of a pixel share an origin and differ by the disk's radius in direction, so a lane group walks the same nodes; a pixel's count is
// the popcount of its group's slice of the ballot of any_hit: no atomics and no LDS. !WAVE: every owner loops over its K rays. A ray's
// boolean comes from the same any_hit on the same (q, d_k) bits in both, so the counts are equal by construction.
// S by value, as in closest_hit.
template <bool WAVE>
NGP_DEV uint32_t sun_disk_count(const MeshSceneParams S, const SunDisk& D, bool owner, f3 q) {
	const uint32_t K = D.n_rays;
	uint32_t count = 0;
	if constexpr (!WAVE) {
		if (owner)
			for (uint32_t k = 0; k < K; ++k) count += any_hit(S, q, ld3(D.d + 3 * k)) ? 1u : 0u;
		return count;
	} else {
		const unsigned long long owners = __ballot(owner);
		const uint32_t n_own = (uint32_t)__popcll(owners), lane = __lane_id();
		const uint32_t per_round = 64u / K, k = lane % K, group = lane / K;
		const uint32_t my_ord = (uint32_t)__popcll(owners & ((1ull << lane) - 1ull)); // an owner's rank among the wave's owners
		const f3 dir = ld3(D.d + 3 * k);
		const unsigned long long slice = (1ull << K) - 1ull; // (K <= 16)
		for (uint32_t base = 0; base < n_own; base += per_round) { // (wave-uniform bounds: every lane takes every shuffle and ballot)
			const uint32_t j = base + group;
			const bool item = j < n_own;
			const int src = (int)nth_set_lane(owners, item ? j : 0u);
			const f3 org = mk3(__shfl(q.x, src), __shfl(q.y, src), __shfl(q.z, src));
			const unsigned long long hits = __ballot(item && any_hit(S, org, dir));
			if (owner && my_ord >= base && my_ord < base + per_round) count = (uint32_t)__popcll((hits >> ((my_ord - base) * K)) & slice);
		}
		return count;
	}
}

// one thread a pixel on the frame's pixel map. A pixel owns a disk where it is covered (plane 1's w) and its primary ray found a triangle
// (plane 2's w); q = mirror_ray's q, the shadow list's bits. V = (K - count) / K, exact for these K, goes over plane 0's w; the pixel's entry
// of the shadow list is rewritten: live (origin q, t = (t_min, +inf), the central direction it has) where V > 0, else dead (origin 0,
// t = (0, 0)). record: (q, 1 + count); the host cleared it, and every other pixel leaves it so. A covered pixel without a hit keeps M4's.
template <bool WAVE>
__global__ void mesh_sun_disk_kernel(const MeshSceneParams S, const CameraParams C, const FrameLayout L, const SunDisk D, float t_min, float4* __restrict__ gbuf,
                                     float* __restrict__ ray_o, float2* __restrict__ ray_t, float4* __restrict__ record) {
	uint32_t x, y, idx;
	const bool mine = frame_pixel(L, C, x, y, idx);
	bool owner = false;
	f3 q = mk3(0.f, 0.f, 0.f);
	if (mine) {
		const float4 g1 = gbuf[(size_t)L.n_pixels + idx];
		if (g1.w != 0.0f) { // (a pixel that is not covered may hold a stale plane 2)
			const float4 g2 = gbuf[2 * (size_t)L.n_pixels + idx];
			if (g2.w != 0.0f) {
				const float4 g0 = gbuf[idx];
				f3 r;
				float c;
				mirror_ray(mk3(g0.x, g0.y, g0.z), mk3(g1.x, g1.y, g1.z), mk3(g2.x, g2.y, g2.z), q, r, c);
				owner = true;
			}
		}
	}
	const uint32_t count = sun_disk_count<WAVE>(S, D, owner, q);
	if (!owner) return;
	const float V = (float)(D.n_rays - count) / (float)D.n_rays;
	gbuf[idx].w = V;
	const bool live = V > 0.0f;
	st3(ray_o + 3 * (size_t)idx, live ? q : mk3(0.f, 0.f, 0.f));
	ray_t[idx] = live ? make_float2(t_min, __builtin_huge_valf()) : make_float2(0.0f, 0.0f);
	record[idx] = make_float4(q.x, q.y, q.z, 1.0f + (float)count);
}

// nerf_mesh_shadow_kernel with the disk: owner, p and q = p + bias shadow_ray_dir(P) as there; f = 1 - strength (count / K), each operation
// rounded, so count = K gives that kernel's f as bits and count = 0 its open pixel; record: (p, 1 + count / K).
template <bool WAVE>
__global__ void nerf_mesh_soft_shadow_kernel(const MeshSceneParams S, const MeshShadeParams P, const ModelParams M, const CameraParams C, float4* __restrict__ frame_buffer,
                                             const float* __restrict__ depth_buffer, const float4* __restrict__ nerf, float4* __restrict__ record, const FrameLayout L,
                                             const SunDisk D, float strength, float bias) {
	uint32_t x, y, idx;
	const bool mine = frame_pixel(L, C, x, y, idx);
	float4 n = make_float4(0.f, 0.f, 0.f, 0.f);
	if (mine) n = nerf[idx];
	const bool owner = n.w > 0.2f;
	f3 p = mk3(0.f, 0.f, 0.f), q = p;
	if (owner) {
		p = nerf_surface_point(M, C, x, y, depth_buffer[idx]);
		q = add3(p, scale3(shadow_ray_dir(P), bias));
	}
	const uint32_t count = sun_disk_count<WAVE>(S, D, owner, q);
	if (n.w == 0.0f) return; // the NeRF pass wrote nothing here (or the pixel is not this launch's): it stays the mesh pass's
	float f = 1.0f;
	if (owner) {
		const float blocked = (float)count / (float)D.n_rays;
		f = 1.0f - strength * blocked;
		record[idx] = make_float4(p.x, p.y, p.z, 1.0f + blocked);
	}
	frame_buffer[idx] = nerf_over_mesh(frame_buffer[idx], n, f);
}

// wave: the layout that deals a pixel's rays over adjacent lanes; else one thread a pixel loops over its rays (the same integers)
void launch_mesh_sun_disk(const MeshSceneParams& S, const CameraParams& C, const FrameLayout& L, const SunDisk& D, bool wave, float t_min, float4* gbuf, float* ray_o,
                          float2* ray_t, float4* record, hipStream_t stream) {
	if (wave) hipLaunchKernelGGL(mesh_sun_disk_kernel<true>, pixel_blocks(C), pixel_threads(), 0, stream, S, C, L, D, t_min, gbuf, ray_o, ray_t, record);
	else hipLaunchKernelGGL(mesh_sun_disk_kernel<false>, pixel_blocks(C), pixel_threads(), 0, stream, S, C, L, D, t_min, gbuf, ray_o, ray_t, record);
}
void launch_nerf_mesh_soft_shadow(const MeshSceneParams& S, const MeshShadeParams& P, const ModelParams& M, const CameraParams& C, float4* frame_buffer,
                                  const float* depth_buffer, const float4* nerf, float4* record, const FrameLayout& L, const SunDisk& D, bool wave, float strength, float bias,
                                  hipStream_t stream) {
	if (wave) hipLaunchKernelGGL(nerf_mesh_soft_shadow_kernel<true>, pixel_blocks(C), pixel_threads(), 0, stream, S, P, M, C, frame_buffer, depth_buffer, nerf, record, L, D, strength, bias);
	else hipLaunchKernelGGL(nerf_mesh_soft_shadow_kernel<false>, pixel_blocks(C), pixel_threads(), 0, stream, S, P, M, C, frame_buffer, depth_buffer, nerf, record, L, D, strength, bias);
}

// ---- the meshes seen by the mirror ray (ngp_set_mesh_reflection_meshes; contract in include/ngp_hip.h, "mesh reflection"). One thread a
// pixel on the frame's pixel map, between mesh_reflection_rays_kernel and the list's prep step: ray_d still holds r as mirror_ray formed it
// and ray_t = (t_min, t_hit), so normalize3(r) has the bits closest_hit was given. A pixel owns a hit where hit_ids names a mesh. For it:
// p2 = q + r^ t_hit; n2 the triangle's raw winding normal (trace_mesh's expression, what M2 hands M5); q2 = p2 + 1e-3 normalize(n2 turned
// against r^) (M3's lift); shadow2 = 0 where any mesh stands between q2 and the sun (nerf_mesh_shadow_kernel's all-meshes rule, not M3's
// one-mesh rule), else 1; C2 = M5 at (p2, n2) viewed along r^. hits: (p2, shadow2), (C2, 1); zeros for every other pixel.
// A kernel of its own: a second M5 inside mesh_shade_deferred_kernel would hold two lookups' accumulators at once.
// MAT (the material instantiation): C2 takes the material of the mesh the mirror ray hit, hit_ids.x (mesh_material_of).
template <bool MAT, typename Ambient>
NGP_DEV void mesh_reflection_hit_shade_body(const MeshSceneParams S, const MeshShadeParams P, const Ambient A, const CameraParams C, const FrameLayout L,
                                            const float* __restrict__ ray_o, const float* __restrict__ ray_d, const float2* __restrict__ ray_t,
                                            const int2* __restrict__ hit_ids, float4* __restrict__ hits, const MeshMaterial* __restrict__ materials) {
	uint32_t x, y, idx;
	if (!frame_pixel(L, C, x, y, idx)) return;
	float4 h0 = make_float4(0.f, 0.f, 0.f, 0.f), h1 = h0;
	const int2 id = hit_ids[idx];
	if (id.x > -1) {
		const f3 q = ld3(ray_o + 3 * (size_t)idx);
		const f3 rh = normalize3(ld3(ray_d + 3 * (size_t)idx));
		const f3 p2 = add3(q, scale3(rh, ray_t[idx].y));
		const Triangle& tri = S.meshes[id.x].tris[id.y];
		const f3 a = ld3(tri.a);
		const f3 n2 = normalize3(cross3(sub3(ld3(tri.b), a), sub3(ld3(tri.c), a)));
		const f3 ff2 = dot3(n2, rh) < 0.0f ? n2 : scale3(n2, -1.0f);
		const f3 q2 = add3(p2, scale3(normalize3(ff2), 1e-3f));
		const float shadow2 = any_hit(S, q2, shadow_ray_dir(P)) ? 0.0f : 1.0f;
		f3 C2;
		if constexpr (MAT) C2 = mesh_shade(mesh_material_of(P, materials, id.x), A, p2, n2, rh, shadow2);
		else C2 = mesh_shade(P, A, p2, n2, rh, shadow2);
		h0 = make_float4(p2.x, p2.y, p2.z, shadow2);
		h1 = make_float4(C2.x, C2.y, C2.z, 1.0f);
	}
	hits[2 * (size_t)idx] = h0;
	hits[2 * (size_t)idx + 1] = h1;
}
template <typename Ambient>
__global__ void mesh_reflection_hit_shade_kernel(const MeshSceneParams S, const MeshShadeParams P, const Ambient A, const CameraParams C, const FrameLayout L,
                                                 const float* __restrict__ ray_o, const float* __restrict__ ray_d, const float2* __restrict__ ray_t,
                                                 const int2* __restrict__ hit_ids, float4* __restrict__ hits) {
	mesh_reflection_hit_shade_body<false>(S, P, A, C, L, ray_o, ray_d, ray_t, hit_ids, hits, nullptr);
}
template <typename Ambient>
__global__ void mesh_reflection_hit_shade_materials_kernel(const MeshSceneParams S, const MeshShadeParams P, const Ambient A, const CameraParams C, const FrameLayout L,
                                                           const float* __restrict__ ray_o, const float* __restrict__ ray_d, const float2* __restrict__ ray_t,
                                                           const int2* __restrict__ hit_ids, float4* __restrict__ hits, const MeshMaterial* __restrict__ materials) {
	mesh_reflection_hit_shade_body<true>(S, P, A, C, L, ray_o, ray_d, ray_t, hit_ids, hits, materials);
}
void launch_mesh_reflection_hit_shade(const MeshSceneParams& S, const MeshShadeParams& P, const IrradianceMap& I, const IrradianceVolume* V, const IrradianceVolumeVisible* VV,
                                      const CameraParams& C, const FrameLayout& L, const float* ray_o, const float* ray_d, const float2* ray_t, const int2* hit_ids, float4* hits,
                                      const MeshMaterial* materials, hipStream_t stream) {
	with_ambient(I, V, VV, [&](const auto& A) {
		if (materials)
			hipLaunchKernelGGL(HIP_KERNEL_NAME(mesh_reflection_hit_shade_materials_kernel<std::decay_t<decltype(A)>>), pixel_blocks(C), pixel_threads(), 0, stream, S, P, A, C, L, ray_o,
			                   ray_d, ray_t, hit_ids, hits, materials);
		else
			hipLaunchKernelGGL(HIP_KERNEL_NAME(mesh_reflection_hit_shade_kernel<std::decay_t<decltype(A)>>), pixel_blocks(C), pixel_threads(), 0, stream, S, P, A, C, L, ray_o, ray_d,
			                   ray_t, hit_ids, hits);
	});
}

// ---- what the meshes change in the ambient light on the NeRF (ngp_set_ambient_change_on_nerf; contract in include/ngp_hip.h, "ambient").
// g = E_after / E_before per channel at (p, n^): both lookups are the plain irradiance_volume_lookup (no visibility maps), `after` the
// context's volume and `before` the reference. a = max(E_after, 0), b = E_before, g = b > min_irradiance ? min(a / b, max_gain) : 1.
// Returns the state: 1 "no estimate" (W_after = 0 or W_before = 0; g = 1), else 2. Identical records in the two volumes give a and b the
// same bits (one lookup function, the same statements) and a / b = 1 exactly, whatever n^ is. The one definition: the stage kernel and
// the frame's ratio kernel both call it.
NGP_DEV float irradiance_volume_ratio(const IrradianceVolume& after, const IrradianceVolume& before, f3 p, f3 nh, float min_irradiance, float max_gain, float (&g)[3],
                                      float& W_after, float& W_before) {
	float Ea[3], Eb[3];
	irradiance_volume_lookup(after, p, nh, Ea, W_after);
	irradiance_volume_lookup(before, p, nh, Eb, W_before);
	g[0] = g[1] = g[2] = 1.0f;
	if (W_after == 0.0f || W_before == 0.0f) return 1.0f;
#pragma unroll
	for (int c = 0; c < 3; ++c) {
		const float a = fmaxf(Ea[c], 0.0f), b = Eb[c];
		if (b > min_irradiance) g[c] = fminf(a / b, max_gain);
	}
	return 2.0f;
}
// one thread per point: out = (g rgb, state) at the point and its normalised normal (ngp_irradiance_volume_ratio)
__global__ void irradiance_volume_ratio_kernel(const IrradianceVolume after, const IrradianceVolume before, uint32_t n, const float* __restrict__ positions,
                                               const float* __restrict__ normals, float min_irradiance, float max_gain, float4* __restrict__ out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	float g[3], Wa, Wb;
	const float state = irradiance_volume_ratio(after, before, ld3(positions + 3 * (size_t)i), normalize3(ld3(normals + 3 * (size_t)i)), min_irradiance, max_gain, g, Wa, Wb);
	out[i] = make_float4(g[0], g[1], g[2], state);
}
// one thread per pixel of the frame's own order: the record nerf_surface_normals_kernel left is (p, state), (N, 0), (1, 1, 1, 0) where the
// pixel owns a surface point (state 2: N is a unit normal; 1: the gradient gave none) and zeros elsewhere. Where N stands, g scales the
// NeRF's colour in the scratch in place and the record becomes (p, state), (N, W_after), (g, W_before).
__global__ void nerf_ambient_ratio_kernel(const IrradianceVolume after, const IrradianceVolume before, uint32_t n_pixels, float4* __restrict__ nerf,
                                          float4* __restrict__ record, float min_irradiance, float max_gain) {
	const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= n_pixels) return;
	const float4 r0 = record[3 * (size_t)idx];
	if (r0.w != 2.0f) return;
	const float4 r1 = record[3 * (size_t)idx + 1];
	float g[3], Wa, Wb;
	const float state = irradiance_volume_ratio(after, before, mk3(r0.x, r0.y, r0.z), mk3(r1.x, r1.y, r1.z), min_irradiance, max_gain, g, Wa, Wb);
	float4 n = nerf[idx];
	n.x *= g[0]; n.y *= g[1]; n.z *= g[2];
	nerf[idx] = n;
	record[3 * (size_t)idx] = make_float4(r0.x, r0.y, r0.z, state);
	record[3 * (size_t)idx + 1] = make_float4(r1.x, r1.y, r1.z, Wa);
	record[3 * (size_t)idx + 2] = make_float4(g[0], g[1], g[2], Wb);
}
// the closing composite of such a frame while ngp_set_mesh_shadow_on_nerf is off: nerf_mesh_shadow_kernel's expression with f = 1, no
// traversal and no record
__global__ void nerf_composite_kernel(const CameraParams C, float4* __restrict__ frame_buffer, const float4* __restrict__ nerf, const FrameLayout L) {
	uint32_t x, y, idx;
	if (!frame_pixel(L, C, x, y, idx)) return;
	const float4 n = nerf[idx];
	if (n.w == 0.0f) return; // the NeRF pass wrote nothing here: the pixel stays the mesh pass's
	frame_buffer[idx] = nerf_over_mesh(frame_buffer[idx], n, 1.0f);
}

void launch_irradiance_volume_ratio(const IrradianceVolume& after, const IrradianceVolume& before, uint32_t n, const float* positions, const float* normals, float min_irradiance,
                                    float max_gain, float4* out, hipStream_t stream) {
	if (n) hipLaunchKernelGGL(irradiance_volume_ratio_kernel, dim3((n + 127) / 128), dim3(128), 0, stream, after, before, n, positions, normals, min_irradiance, max_gain, out);
}
void launch_nerf_ambient_ratio(const IrradianceVolume& after, const IrradianceVolume& before, uint32_t n_pixels, float4* nerf, float4* record, float min_irradiance,
                               float max_gain, hipStream_t stream) {
	if (n_pixels) hipLaunchKernelGGL(nerf_ambient_ratio_kernel, dim3((n_pixels + 127) / 128), dim3(128), 0, stream, after, before, n_pixels, nerf, record, min_irradiance, max_gain);
}
void launch_nerf_composite(const CameraParams& C, float4* frame_buffer, const float4* nerf, const FrameLayout& L, hipStream_t stream) {
	hipLaunchKernelGGL(nerf_composite_kernel, pixel_blocks(C), pixel_threads(), 0, stream, C, frame_buffer, nerf, L);
}

} // namespace ngp
