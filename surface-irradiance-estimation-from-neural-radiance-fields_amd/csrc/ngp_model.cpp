// The model behind a context: descriptor validation, the device tables of both architectures (hash grid in tcnn order and
// in the xor layout, MFMA weight fragments), the occupancy grid and its refresh.
#include "ngp_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace ngp;

namespace {

uint32_t next_multiple(uint32_t v, uint32_t d) { return ((v + d - 1) / d) * d; }

// tcnn GridEncoding level table
void build_levels(const ngp_model_desc& d, LevelInfo* lv, uint32_t* total_entries) {
	float log2_pls = log2f(d.per_level_scale);
	uint32_t offset = 0;
	for (uint32_t l = 0; l < d.n_levels; ++l) {
		float scale = exp2f((float)l * log2_pls) * (float)d.base_resolution - 1.0f;
		if (!(scale >= 0.0f && scale < 1073741824.0f)) throw std::runtime_error("invalid hash grid configuration (a level's resolution is out of range)");
		uint32_t res = (uint32_t)ceilf(scale) + 1u;
		uint32_t max_params = 0xFFFFFFFFu / 2u;
		uint32_t n = powf((float)res, 3.0f) > (float)max_params ? max_params : res * res * res;
		n = next_multiple(n, 8u);
		n = std::min(n, 1u << d.log2_hashmap_size);
		// grid_index: strides accumulate while stride <= size; hashed iff the final stride exceeds the level size
		uint32_t stride = 1;
		for (int dim = 0; dim < 3 && stride <= n; ++dim) stride *= res;
		lv[l].scale = scale;
		lv[l].res = res;
		lv[l].size = n;
		lv[l].offset = offset;
		lv[l].hashed = n < stride ? 1u : 0u;
		lv[l].mask = (n & (n - 1)) == 0 ? n - 1 : 0u;
		lv[l].xor_disabled = 0;
		if ((uint64_t)offset + n > 0x1FFFFFFFull) throw std::runtime_error("grid encoding too large for 32-bit gather offsets (more than 2^29 entries)");
		offset += n;
	}
	*total_entries = offset;
}

// Xor layout of the hash-grid table for the render kernels. tcnn's grid_index has two shapes -- a dense
// x + y*res + z*res^2 (wrapped modulo the level size when a corner coordinate reaches res) and a prime-multiplier
// xor hash -- and the two halves of a wave work on levels of different shape. Dense levels are therefore re-laid
// out at load time with power-of-two strides, entry (x, y, z) at x | y << b | z << 2b for x, y, z in [0, res],
// 2^b > res, each holding the entry tcnn's formula (including its wrap) would have fetched; then
//   dense:  8x ^ y * (8 << b) ^ z * (8 << 2b)        (disjoint bit fields: xor == add)
//   hashed: 8x ^ y * (8 * 2654435761) ^ z * (8 * 805459861), masked with 8 * (size - 1)
// is ONE formula with per-level multipliers, and aligning every level to its power-of-two footprint turns
// "+ offset" into an OR. Same table entries, so the features are bit-identical; the cost is HBM nobody misses
// (Lego-shaped model: 23 MB -> 38 MB).
uint64_t pow2_ceil(uint64_t v) {
	uint64_t p = 1;
	while (p < v) p <<= 1;
	return p;
}
void build_xor_layout(LevelInfo* lv, uint32_t n_levels, const uint16_t* grid /* tcnn order, 4 halves per entry */, std::vector<uint64_t>& table) {
	uint64_t cursor = 0;
	std::vector<uint32_t> bits(n_levels, 0), wrapped(n_levels, 0);
	for (uint32_t l = 0; l < n_levels; ++l) {
		LevelInfo& L = lv[l];
		uint64_t bytes;
		if (L.hashed) {
			if ((L.size & (L.size - 1)) != 0) throw std::runtime_error("hashed grid level whose size is not a power of two");
			bytes = (uint64_t)L.size * 8u;
		} else if ((uint64_t)L.res * L.res * L.res > (uint64_t)L.size) {
			// tcnn's grid_index forms its strides in uint32: at res = 65536 (level 6 of the upstream aabb_scale-128 configuration,
			// per_level_scale 4) res^2 wraps to 0, the loop's guard `stride <= hashmap_size` keeps going and the level is indexed
			// as (x + y * 65536 + z * 0) % size -- dense by the code's own test, with z dropped. Same entries here: x < res and a
			// power-of-two res keep the fields disjoint (add == xor), so the hashed form serves it with multipliers (res, 0);
			// the corner x + 1 == res would carry into y's field, hence coord_max = res - 2 (beyond it the wave takes
			// level_corners on the tcnn-order table, which wraps exactly like tcnn).
			const bool pow2 = (L.res & (L.res - 1)) == 0 && (L.size & (L.size - 1)) == 0 && L.res * L.res == 0u;
			wrapped[l] = pow2 ? 1 : 2; // 2: no xor form -- every wave takes the tcnn-order table for this level
			bytes = pow2 ? (uint64_t)L.size * 8u : 8u;
		} else {
			uint32_t b = 0;
			while ((1u << b) <= L.res) ++b; // 2^b > res: coordinates 0..res fit
			bits[l] = b;
			bytes = pow2_ceil(((uint64_t)(L.res + 1u) << (2 * b)) * 8u);
		}
		cursor = (cursor + bytes - 1) / bytes * bytes;
		if (cursor + bytes > 0xFFFFFFFFull) throw std::runtime_error("hash grid too large for 32-bit gather offsets");
		L.base8 = (uint32_t)cursor;
		if (L.hashed) {
			L.coord_max = 0xFFFFFFFFu;
			L.mul_y8 = 2654435761u * 8u;
			L.mul_z8 = 805459861u * 8u;
			L.mask8 = (L.size - 1u) * 8u;
		} else if (wrapped[l] == 1) {
			L.coord_max = L.res - 2u;
			L.mul_y8 = L.res * 8u;
			L.mul_z8 = 0u;
			L.mask8 = (L.size - 1u) * 8u;
		} else if (wrapped[l] == 2) {
			L.xor_disabled = 1u;
			L.coord_max = 0u;
			L.mul_y8 = L.mul_z8 = L.mask8 = 0u;
		} else {
			L.coord_max = L.res - 1u;
			L.mul_y8 = 8u << bits[l];
			L.mul_z8 = 8u << (2 * bits[l]);
			L.mask8 = 0xFFFFFFFFu;
		}
		cursor += bytes;
	}
	table.assign(cursor / 8u, 0ull);
	const uint64_t* src = (const uint64_t*)grid;
	for (uint32_t l = 0; l < n_levels; ++l) {
		const LevelInfo& L = lv[l];
		uint64_t* dst = table.data() + L.base8 / 8u;
		const uint64_t* level = src + L.offset;
		if (L.hashed || wrapped[l] == 1) {
			std::copy(level, level + L.size, dst);
			continue;
		}
		if (wrapped[l] == 2) continue;
		const uint32_t b = bits[l];
		for (uint32_t z = 0; z <= L.res; ++z)
			for (uint32_t y = 0; y <= L.res; ++y)
				for (uint32_t x = 0; x <= L.res; ++x) dst[x | (y << b) | (z << (2 * b))] = level[(x + y * L.res + z * L.res * L.res) % L.size];
	}
}

uint64_t mlp_n_params(uint32_t n_in, uint32_t width, uint32_t n_hidden, uint32_t n_out) {
	if (n_hidden == 0) return (uint64_t)n_out * n_in; // tcnn CutlassMLP without a hidden layer: one (padded output) x (input) matrix
	return (uint64_t)width * n_in + (uint64_t)(n_hidden - 1) * width * width + (uint64_t)n_out * width;
}

// MFMA A-operand fragments for v_mfma_f32_16x16x32_f16: fragment (tile m, k-step s) holds, in lane l = (h = l>>4,
// row = l&15), element j: W[16m + row][n(s,h,j)], n(s,h,j) = 32s + 16(j>>2) + 4h + (j&3). The K permutation n() is
// the order in which the previous layer's accumulator tiles (and the encoder's level pairs) already sit in the
// B operand's registers, so no activation ever moves between lanes (nerf_device.h mlp_pass).
// n_out rows are stored (a CutlassMLP's output layer: 8); tiles are filled up with zero rows.
void emit_fragments(std::vector<uint16_t>& frags, int first_frag, const uint16_t* W, int n_out, int n_in) {
	int f = first_frag;
	for (int m = 0; m < (n_out + 15) / 16; ++m) {
		for (int s = 0; s < n_in / 32; ++s, ++f) {
			for (int l = 0; l < 64; ++l) {
				int h = l >> 4, row = l & 15;
				for (int j = 0; j < 8; ++j) {
					int k = 32 * s + 16 * (j >> 2) + 4 * h + (j & 3);
					frags[((size_t)f * 64 + l) * 8 + j] = 16 * m + row < n_out ? W[(size_t)(16 * m + row) * n_in + k] : (uint16_t)0;
				}
			}
		}
	}
}

// MFMA A fragments of one layer of the wide architecture (ngp_kernels.h WideModel): [m tile][k block][lane] x 8 fp16, zeros beyond the matrix
WideLayer emit_wide_fragments(std::vector<uint16_t>& frags, const uint16_t* W, uint32_t n_out, uint32_t n_in) {
	constexpr uint32_t TM = (uint32_t)ngp::WIDE_TILE_M, TK = (uint32_t)ngp::WIDE_TILE_K;
	WideLayer L{};
	L.frag_offset = (uint32_t)(frags.size() / 8);
	L.n_kblocks = (uint16_t)((n_in <= 128 ? 128u : 256u) / TK); // the kernels are instantiated for K = 128 and 256 (zero columns beyond the matrix)
	L.n_mtiles = (uint16_t)((n_out + TM - 1) / TM);
	frags.resize(frags.size() + (size_t)L.n_mtiles * L.n_kblocks * 64 * 8, 0);
	uint16_t* out = frags.data() + (size_t)L.frag_offset * 8;
	for (uint32_t m = 0; m < L.n_mtiles; ++m)
		for (uint32_t kb = 0; kb < L.n_kblocks; ++kb)
			for (uint32_t l = 0; l < 64; ++l)
				for (uint32_t j = 0; j < 8; ++j) {
					const uint32_t row = TM * m + (l % TM), col = TK * kb + 8 * (l / TM) + j;
					if (row < n_out && col < n_in) out[(((size_t)m * L.n_kblocks + kb) * 64 + l) * 8 + j] = W[(size_t)row * n_in + col];
				}
	return L;
}

// widths of the wide architecture as NerfNetwork derives them (nerf_network.h:81-100)
struct WideShapes {
	uint32_t alignment, enc_dims, dir_dims, rgb_in, rgb_out;
};
WideShapes wide_shapes(const ngp_model_desc& d) {
	WideShapes w{};
	w.alignment = d.mlp_alignment ? d.mlp_alignment : 16u;
	auto up = [&](uint32_t v) { return (v + w.alignment - 1) / w.alignment * w.alignment; };
	w.enc_dims = d.pos_encoding == 2 ? up(3u) : up(6u * d.pos_n_frequencies);
	w.dir_dims = d.dir_encoding == 1 ? up(6u * d.dir_n_frequencies) : d.dir_encoding == 2 ? up(3u) : 16u;
	w.rgb_in = up(d.density_out_dims + w.dir_dims);
	w.rgb_out = up(3u);
	return w;
}

// what a valid descriptor implies
struct ModelLayout {
	uint64_t nd, nr, ng; // parameters of the density MLP, of the rgb MLP, of the grid table
	uint32_t max_cascade;
	WideShapes ws;
	LevelInfo levels[N_LEVELS]; // grid models (the xor fields are filled at upload)
};

// every check of a descriptor, before anything of the context changes
ModelLayout validate_model_desc(const ngp_model_desc& d) {
	const bool wide = d.pos_encoding >= 1; // Frequency (1) or Identity (2) position encoding: no grid, the wide-MLP kernels
	if (d.pos_encoding > 2 || d.dir_encoding > 2 || (d.mlp_alignment != 0 && d.mlp_alignment != 8 && d.mlp_alignment != 16)) throw std::runtime_error("invalid model descriptor (encoding kinds / mlp_alignment)");
	if (!wide && d.dir_encoding != 0) throw std::runtime_error("unsupported network architecture: a Frequency / Identity direction encoding is implemented together with a Frequency / Identity position encoding (configs/nerf/frequency.json, none.json)");
	if (wide) {
		if ((d.n_neurons != 128 && d.n_neurons != 256) || d.n_hidden_density < 1 || d.n_hidden_rgb < 1 || d.n_hidden_density + d.n_hidden_rgb + 2 > (uint32_t)WIDE_MAX_LAYERS ||
		    d.density_out_dims != 16 || (d.pos_encoding == 1 && (d.pos_n_frequencies < 1 || d.pos_n_frequencies > 40)) || (d.dir_encoding == 1 && (d.dir_n_frequencies < 1 || d.dir_n_frequencies > 4))) {
			throw std::runtime_error("unsupported network architecture: with a Frequency position encoding (configs/nerf/frequency.json) the HIP path implements MLPs of 128 or 256 "
			                         "neurons with 1 or more hidden layers, a 16-wide density output, up to 40 position and 4 direction frequencies");
		}
	} else if (d.n_levels != N_LEVELS || d.n_features_per_level != N_FEATURES || d.n_neurons != MLP_WIDTH || d.n_hidden_density > 1 ||
	           d.n_hidden_rgb > 1 + (uint32_t)MAX_RGB_MID || d.density_out_dims != 16 || (d.n_hidden_density == 0 && d.n_hidden_rgb != 0)) {
		throw std::runtime_error("unsupported network architecture: the HIP path is specialised for configs/nerf/base.json and its variants "
		                         "(HashGrid 8 levels x 4 features; density MLP 64x1 hidden -> 16 with an rgb MLP 64 wide of 0 to 3 hidden layers -- "
		                         "base, base_0layer .. base_3layer --, or both heads without a hidden layer -- linear.json)");
	}
	if (!wide && ((d.log2_hashmap_size > 28 && d.log2_hashmap_size != 31) || d.base_resolution == 0 || !(d.per_level_scale > 0.f))) throw std::runtime_error("invalid hash grid configuration");
	if (d.aabb_scale == 0 || (d.aabb_scale & (d.aabb_scale - 1)) != 0) throw std::runtime_error("NeRF dataset's `aabb_scale` must be a power of two"); // testbed_nerf.cu:2707
	if (d.aabb_scale > (1u << (NERF_CASCADES - 1))) throw std::runtime_error("NeRF dataset must have `aabb_scale <= 128`"); // :2711-2718

	ModelLayout L{};
	uint32_t total_entries = 0;
	if (!wide) build_levels(d, L.levels, &total_entries);
	L.ws = wide_shapes(d);
	const uint32_t enc_dims = wide ? L.ws.enc_dims : d.n_levels * d.n_features_per_level;
	L.nd = mlp_n_params(enc_dims, d.n_neurons, d.n_hidden_density, d.density_out_dims);
	// (grid models: the rgb input is 16 + 16 wide under either alignment; the output is padded to the rgb network's -- 8 rows for a CutlassMLP)
	L.nr = wide ? mlp_n_params(L.ws.rgb_in, d.n_neurons, d.n_hidden_rgb, L.ws.rgb_out) : mlp_n_params(d.density_out_dims + 16u, d.n_neurons, d.n_hidden_rgb, L.ws.rgb_out);
	L.ng = wide ? 0 : (uint64_t)total_entries * d.n_features_per_level;
	if (d.n_params != L.nd + L.nr + L.ng || !d.params_fp16) {
		throw std::runtime_error("parameter count mismatch: snapshot has " + std::to_string(d.n_params) + ", network needs " + std::to_string(L.nd + L.nr + L.ng));
	}
	while ((1u << L.max_cascade) < d.aabb_scale) ++L.max_cascade; // testbed_nerf.cu:2729-2732
	if (d.n_density_grid != 0 && d.n_density_grid != (uint64_t)NERF_GRID_N_CELLS * (L.max_cascade + 1)) throw std::runtime_error("Incompatible number of grid cascades."); // testbed.cu:5350
	return L;
}

// every layer's weights as MFMA A fragments (wide_kernels.hip)
void upload_wide_weights(ngp_ctx* ctx, const ngp_model_desc& d, const WideShapes& ws, WideModel& WM) {
	std::vector<uint16_t> frags;
	WM.width = d.n_neurons;
	WM.pos_freqs = d.pos_encoding == 1 ? d.pos_n_frequencies : 0u;
	WM.dir_freqs = d.dir_encoding == 1 ? d.dir_n_frequencies : 0u;
	WM.pos_identity = d.pos_encoding == 2 ? 1u : 0u;
	WM.dir_identity = d.dir_encoding == 2 ? 1u : 0u;
	WM.enc_dims = ws.enc_dims;
	WM.dir_dims = ws.dir_dims;
	WM.rgb_in = ws.rgb_in;
	WM.n_hidden_density = d.n_hidden_density;
	WM.n_hidden_rgb = d.n_hidden_rgb;
	const uint16_t* W = ctx->params.data();
	uint32_t l = 0;
	auto emit_mlp = [&](uint32_t n_in, uint32_t n_hidden, uint32_t n_out) {
		WM.layers[l++] = emit_wide_fragments(frags, W, d.n_neurons, n_in);
		W += (size_t)d.n_neurons * n_in;
		for (uint32_t k = 1; k < n_hidden; ++k) {
			WM.layers[l++] = emit_wide_fragments(frags, W, d.n_neurons, d.n_neurons);
			W += (size_t)d.n_neurons * d.n_neurons;
		}
		WM.layers[l++] = emit_wide_fragments(frags, W, n_out, d.n_neurons);
		W += (size_t)n_out * d.n_neurons;
	};
	emit_mlp(ws.enc_dims, d.n_hidden_density, d.density_out_dims);
	emit_mlp(ws.rgb_in, d.n_hidden_rgb, ws.rgb_out);
	if (d.n_hidden_density <= (uint32_t)WIDE_MAX_NORMALS_LAYERS) {
		// ERenderMode::Normals: the density network's hidden layers transposed (the backward pass of tcnn's input_gradient runs the same GEMM
		// kernels on them), zero rows beyond the encoding's width in layer 0, and row 0 of the output layer (the one-hot loss gradient's only row)
		const uint16_t* D = ctx->params.data();
		std::vector<uint16_t> wt((size_t)d.n_neurons * d.n_neurons);
		uint32_t n_in = ws.enc_dims;
		for (uint32_t k = 0; k < d.n_hidden_density; ++k) {
			std::fill(wt.begin(), wt.end(), (uint16_t)0);
			for (uint32_t o = 0; o < d.n_neurons; ++o)
				for (uint32_t i = 0; i < n_in && i < d.n_neurons; ++i) wt[(size_t)i * d.n_neurons + o] = D[(size_t)o * n_in + i];
			WM.layers_t[k] = emit_wide_fragments(frags, wt.data(), d.n_neurons, d.n_neurons);
			D += (size_t)d.n_neurons * n_in;
			n_in = d.n_neurons;
		}
		WM.out_row0_offset = (uint32_t)(frags.size() / 8);
		frags.insert(frags.end(), D, D + d.n_neurons); // (D now points at the output layer: row 0 = the density logit's weights)
	}
	ctx->d_wfrags.upload((const uint4*)frags.data(), frags.size() / 8);
	WM.frags = ctx->d_wfrags.get();
}

// a grid model's tables: the hash grid in tcnn order and in the xor layout, the weight fragments of the two MLPs
void upload_grid_tables(ngp_ctx* ctx, const ngp_model_desc& d, const ModelLayout& L, ModelParams& M) {
	const uint64_t nd = L.nd, nr = L.nr, ng = L.ng;
	memcpy(M.levels, L.levels, sizeof(M.levels));
	// grid table
	ctx->d_params.upload(ctx->params.data() + nd + nr, ng);
	{
		std::vector<uint64_t> table;
		build_xor_layout(M.levels, d.n_levels, ctx->params.data() + nd + nr, table);
		ctx->d_xgrid.upload(table.data(), table.size());
		if (table.size() * sizeof(uint64_t) > 0x7FFFFFFFull || ng * sizeof(uint16_t) > 0x7FFFFFFFull) throw std::runtime_error("hash grid too large for 31-bit buffer-load offsets");
		M.xgrid_bytes = (uint32_t)(table.size() * sizeof(uint64_t));
		M.grid_bytes = (uint32_t)(ng * sizeof(uint16_t));
	}
	// weight fragments
	std::vector<uint16_t> frags((size_t)(N_FRAGS_MAX + N_NORMALS_FRAGS) * 64 * 8, 0); // (the Normals mode's four are permuted out of the forward ones on the device, below)
	const uint16_t* W = ctx->params.data();
	if (d.n_hidden_density == 0) {
		emit_fragments(frags, FRAG_D0, W, 16, 32); // configs/nerf/linear.json: the 16 x 32 output layer alone
	} else {
		emit_fragments(frags, FRAG_D0, W, 64, 32);
		emit_fragments(frags, FRAG_D1, W + 64 * 32, 16, 64);
	}
	const uint16_t* R = W + nd;
	const int rgb_mid = (int)d.n_hidden_rgb - 1; // 64x64 layers between the first and the output layer of the rgb head; -1: the output layer alone
	if (rgb_mid < 0) {
		emit_fragments(frags, FRAG_R0, R, (int)L.ws.rgb_out, 32);
	} else {
		emit_fragments(frags, FRAG_R0, R, 64, 32);
		for (int k = 0; k < rgb_mid; ++k) emit_fragments(frags, FRAG_R1 + 8 * k, R + 64 * 32 + (size_t)k * 64 * 64, 64, 64);
		emit_fragments(frags, FRAG_R1 + 8 * rgb_mid, R + 64 * 32 + (size_t)rgb_mid * 64 * 64, (int)L.ws.rgb_out, 64);
	}
	M.rgb_mid = rgb_mid;
	M.density_linear = d.n_hidden_density == 0 ? 1u : 0u;
	ctx->d_wfrags.upload((const uint4*)frags.data(), frags.size() / 8);
	launch_build_normals_fragments(ctx->d_wfrags.get(), ctx->stream);
}

// occupancy: fp16 grid -> fp32 -> bitfield + mips on the device (K8/K9)
void upload_occupancy(ngp_ctx* ctx, const ngp_model_desc& d, uint32_t max_cascade) {
	const uint64_t n_grid_expected = (uint64_t)NERF_GRID_N_CELLS * (max_cascade + 1);
	const size_t bitfield_bytes = (size_t)NERF_GRID_N_CELLS / 8 * NERF_CASCADES;
	ctx->d_bitfield.reset(bitfield_bytes);
	ctx->d_density_f32.reset(n_grid_expected);
	ctx->d_partial.reset(256);
	if (d.n_density_grid) {
		ctx->d_density_f16.upload(ctx->density_grid.data(), d.n_density_grid);
	} else {
		// a snapshot whose grid was never populated renders as empty space (testbed.cu:5348-5351)
		NGP_HIP_CHECK(hipMemset(ctx->d_density_f32.get(), 0, n_grid_expected * sizeof(float)));
	}
	launch_density_grid_to_bitfield(ctx->d_density_f16.get(), (uint32_t)d.n_density_grid, max_cascade, ctx->d_density_f32.get(), ctx->d_partial.get(), ctx->d_bitfield.get(),
	                                &ctx->bitfield_mean, ctx->stream);
	ctx->d_coarse.reset((size_t)COARSE_TOTAL_WORDS); // both summaries and the block words (occ_index.h)
	launch_coarse_occupancy(ctx->d_bitfield.get(), ctx->d_coarse.get(), ctx->stream);
	NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	NGP_HIP_CHECK(hipGetLastError());
}

// the device tables' addresses and the by-value render state of the descriptor
void fill_model_params(const ngp_ctx* ctx, const ngp_model_desc& d, uint32_t max_cascade, ModelParams& M) {
	M.grid = (const uint2*)ctx->d_params.get();
	M.xgrid = (const char*)ctx->d_xgrid.get();
	M.coarse = ctx->d_coarse.get();
	M.wfrags = d.pos_encoding >= 1 ? nullptr : ctx->d_wfrags.get();
	M.bitfield = ctx->d_bitfield.get();
	for (int i = 0; i < 3; ++i) {
		M.aabb_min[i] = d.aabb_min[i];
		M.aabb_diag[i] = d.aabb_max[i] - d.aabb_min[i];
		M.raabb_min[i] = d.render_aabb_min[i];
		M.raabb_max[i] = d.render_aabb_max[i];
	}
	for (int i = 0; i < 9; ++i) M.r2l[i] = d.render_aabb_to_local[i];
	{
		const float ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
		M.r2l_identity = memcmp(M.r2l, ident, sizeof(ident)) == 0 ? 1u : 0u;
		M.diag_pow2 = 1u;
		for (int i = 0; i < 3; ++i) {
			int e;
			float m = frexpf(M.aabb_diag[i], &e);
			if (!(m == 0.5f) || e < -100 || e > 100) M.diag_pow2 = 0u; // power of two, comfortably inside the normal range
			M.aabb_inv_diag[i] = 1.0f / M.aabb_diag[i];
		}
	}
	M.max_cascade = max_cascade;
	M.cone_angle = d.cone_angle_constant;
	M.rgb_act = d.rgb_activation;
	M.density_act = d.density_activation;
}

} // namespace

namespace ngp {
void free_model(ngp_ctx* ctx) {
	free_training(ctx);
	ctx->d_params.reset();
	ctx->d_xgrid.reset();
	ctx->d_wfrags.reset();
	ctx->d_bitfield.reset();
	ctx->d_coarse.reset();
	ctx->d_density_f16.reset();
	ctx->d_density_f32.reset();
	ctx->d_density_tmp.reset();
	ctx->d_partial.reset();
	ctx->model_loaded = false;
}

// validate, then replace the context's model: host copies, device tables, occupancy, render parameters
void set_model_impl(ngp_ctx* ctx, const ngp_model_desc& d) {
	const ModelLayout L = validate_model_desc(d);

	if (ctx->device >= 0) NGP_HIP_CHECK(hipDeviceSynchronize()); // frames in flight read the tables about to be freed
	free_model(ctx);
	ctx->params.assign(d.params_fp16, d.params_fp16 + d.n_params);
	ctx->density_grid.assign(d.density_grid_fp16, d.density_grid_fp16 + d.n_density_grid);
	ctx->desc = d;
	ctx->desc.params_fp16 = nullptr;
	ctx->desc.density_grid_fp16 = nullptr;
	ctx->max_cascade = L.max_cascade;
	ctx->have_desc = true;
	{ // reset_network: m_rng = default_rng_t{m_seed}; density_grid_rng = default_rng_t{m_rng.next_uint()} (testbed.cu:3848-3861, m_seed = 1337)
		Pcg32 rng;
		rng.seed(1337u);
		Pcg32 grid_rng;
		grid_rng.seed(rng.next_uint());
		ctx->grid_rng_state = grid_rng.state;
		ctx->grid_rng_inc = grid_rng.inc;
		ctx->grid_ema_step = 0;
		ctx->grid_updates = 0;
	}
	if (ctx->device < 0) return; // host-only context: the model is parsed and validated, nothing can be rendered

	ModelParams M{};
	if (d.pos_encoding >= 1) upload_wide_weights(ctx, d, L.ws, M.wide);
	else upload_grid_tables(ctx, d, L, M);
	upload_occupancy(ctx, d, L.max_cascade);
	fill_model_params(ctx, d, L.max_cascade, M);
	ctx->M = M;
	ctx->model_loaded = true;
	++ctx->model_generation;
	ctx->grid_generation = ctx->params_generation = 0;
}

void update_density_grid_device(ngp_ctx* ctx, float decay, uint32_t n_uniform, uint32_t n_nonuniform, uint32_t n_iterations) {
	const uint32_t n_cascades = ctx->max_cascade + 1;
	const uint32_t n_elements = NERF_GRID_N_CELLS * n_cascades;
	hipStream_t stream = ctx->stream;
	ensure_frame_buffers(ctx, 0);
	order_after_frames(ctx, stream); // frames in flight on ANY stream read the bitfield and its summaries: the refresh waits for them on the device
	if (!ctx->d_density_tmp) ctx->d_density_tmp.reset(n_elements);
	Pcg32 rng;
	rng.state = ctx->grid_rng_state;
	rng.inc = ctx->grid_rng_inc;
	for (uint32_t it = 0; it < n_iterations; ++it) {
		uint32_t nu = n_uniform, nn = n_nonuniform;
		if (nu == 0 && nn == 0) { // training_prep_nerf's schedule (src/testbed_nerf.cu:3441-3445)
			if (ctx->grid_updates < 256) nu = NERF_GRID_N_CELLS * n_cascades;
			else nu = nn = NERF_GRID_N_CELLS / 4 * n_cascades;
		}
		NGP_HIP_CHECK(hipMemsetAsync(ctx->d_density_tmp.get(), 0, (size_t)n_elements * sizeof(float), stream));
		if (ctx->M.wide.width) { // a network without a hash grid: positions -> NerfNetwork::inference (wide_kernels.hip) -> splat
			const size_t n_max = std::max(nu, nn);
			if (n_max * 24 > ctx->d_grid_scratch.size()) ctx->d_grid_scratch.reset(n_max * 24);
			float* d_pos = (float*)ctx->d_grid_scratch.get();
			uint32_t* d_cell = (uint32_t*)(ctx->d_grid_scratch.get() + n_max * 12);
			uint16_t* d_out = (uint16_t*)(ctx->d_grid_scratch.get() + n_max * 16);
			launch_density_grid_update_wide(ctx->M, nu, rng, ctx->grid_ema_step, n_cascades, -0.01f, ctx->d_density_f32.get(), ctx->d_density_tmp.get(), d_pos, d_cell, d_out, ctx->n_cus, stream);
			rng.advance();
			launch_density_grid_update_wide(ctx->M, nn, rng, ctx->grid_ema_step, n_cascades, 0.01f, ctx->d_density_f32.get(), ctx->d_density_tmp.get(), d_pos, d_cell, d_out, ctx->n_cus, stream);
			rng.advance();
		} else {
			launch_density_grid_update(ctx->M, nu, rng, ctx->grid_ema_step, n_cascades, -0.01f, ctx->d_density_f32.get(), ctx->d_density_tmp.get(), stream);
			rng.advance();
			launch_density_grid_update(ctx->M, nn, rng, ctx->grid_ema_step, n_cascades, 0.01f /* NERF_MIN_OPTICAL_THICKNESS */, ctx->d_density_f32.get(), ctx->d_density_tmp.get(), stream);
			rng.advance();
		}
		launch_density_grid_ema(n_elements, decay, ctx->d_density_f32.get(), ctx->d_density_tmp.get(), stream);
		++ctx->grid_ema_step;
		++ctx->grid_updates;
	}
	ctx->grid_rng_state = rng.state;
	ctx->grid_rng_inc = rng.inc;
	// update_density_grid_mean_and_bitfield (:2863-2880) + the block summaries the march reads
	launch_density_grid_to_bitfield(nullptr, 0, ctx->max_cascade, ctx->d_density_f32.get(), ctx->d_partial.get(), ctx->d_bitfield.get(), &ctx->bitfield_mean, stream);
	launch_coarse_occupancy(ctx->d_bitfield.get(), ctx->d_coarse.get(), stream);
	mark_model_updated(ctx, stream);
	ctx->density_grid_host_dirty = true;
	++ctx->grid_generation;
}
// keep the snapshot copy (fp16, as the reference serialises it) in step
void refresh_density_grid_host(ngp_ctx* ctx) {
	if (!ctx->density_grid_host_dirty || ctx->device < 0 || !ctx->model_loaded) return;
	const uint32_t n_elements = NERF_GRID_N_CELLS * (ctx->max_cascade + 1);
	std::vector<float> grid(n_elements);
	NGP_HIP_CHECK(hipMemcpyAsync(grid.data(), ctx->d_density_f32.get(), (size_t)n_elements * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
	NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	NGP_HIP_CHECK(hipGetLastError());
	ctx->density_grid.resize(n_elements);
	for (uint32_t i = 0; i < n_elements; ++i) ctx->density_grid[i] = float_to_half(grid[i]);
	ctx->desc.n_density_grid = n_elements;
	ctx->density_grid_host_dirty = false;
}
} // namespace ngp

// ================================================================================================== C ABI
extern "C" {

int ngp_set_model(ngp_ctx* ctx, const ngp_model_desc* desc) {
	return guarded(ctx, [&] {
		if (!desc) throw std::runtime_error("null model descriptor");
		set_model_impl(ctx, *desc);
		ctx->config = mj::Value();
	});
}

int ngp_get_model(ngp_ctx* ctx, ngp_model_desc* out) {
	if (!ctx || !out || !ctx->have_desc) return -1;
	return guarded(ctx, [&] {
		if (ctx->device >= 0) { // what was trained / refreshed on the device since is part of "the model as currently loaded"
			ngp::sync_host_params(ctx);
			ngp::refresh_density_grid_host(ctx);
		}
		*out = ctx->desc;
		out->params_fp16 = ctx->params.data();
		out->n_params = ctx->params.size();
		out->density_grid_fp16 = ctx->density_grid.data();
		out->n_density_grid = ctx->density_grid.size();
	});
}

int ngp_set_render_aabb(ngp_ctx* ctx, const float* min3, const float* max3, const float* to_local9) {
	return guarded(ctx, [&] {
		if (!ctx->have_desc) throw std::runtime_error("No network available.");
		if (!min3 || !max3) throw std::runtime_error("null argument");
		for (int i = 0; i < 3; ++i) if (!(min3[i] <= max3[i])) throw std::runtime_error("render_aabb: min must not exceed max");
		if (ctx->last_stream) NGP_HIP_CHECK(hipStreamSynchronize(ctx->last_stream));
		const float ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
		const float* r2l = to_local9 ? to_local9 : ident;
		memcpy(ctx->desc.render_aabb_min, min3, 12);
		memcpy(ctx->desc.render_aabb_max, max3, 12);
		memcpy(ctx->desc.render_aabb_to_local, r2l, 36);
		memcpy(ctx->M.raabb_min, min3, 12);
		memcpy(ctx->M.raabb_max, max3, 12);
		memcpy(ctx->M.r2l, r2l, 36);
		ctx->M.r2l_identity = memcmp(r2l, ident, 36) == 0 ? 1u : 0u;
	});
}

int ngp_set_cone_angle_constant(ngp_ctx* ctx, float cone_angle_constant) {
	return guarded(ctx, [&] {
		if (!ctx->have_desc) throw std::runtime_error("No network available.");
		if (!(cone_angle_constant >= 0.f)) throw std::runtime_error("cone_angle_constant must be >= 0");
		if (ctx->last_stream) NGP_HIP_CHECK(hipStreamSynchronize(ctx->last_stream));
		ctx->desc.cone_angle_constant = cone_angle_constant;
		ctx->M.cone_angle = cone_angle_constant;
	});
}

int ngp_update_density_grid(ngp_ctx* ctx, float decay, uint32_t n_uniform, uint32_t n_nonuniform, uint32_t n_iterations) {
	return guarded(ctx, [&] {
		require_model(ctx);
		ngp::sync_inference_model(ctx);
		ngp::update_density_grid_device(ctx, decay, n_uniform, n_nonuniform, n_iterations);
		ngp::refresh_density_grid_host(ctx);
	});
}

int ngp_get_density_grid(ngp_ctx* ctx, float* out, uint64_t n) {
	return guarded(ctx, [&] {
		require_model(ctx);
		ngp::sync_inference_model(ctx);
		const uint64_t n_elements = (uint64_t)NERF_GRID_N_CELLS * (ctx->max_cascade + 1);
		if (!out || n != n_elements) throw std::runtime_error("density grid holds " + std::to_string(n_elements) + " values");
		NGP_HIP_CHECK(hipMemcpy(out, ctx->d_density_f32.get(), n_elements * sizeof(float), hipMemcpyDeviceToHost));
	});
}

} // extern "C"
