// C ABI of libngp_hip (include/ngp_hip.h): contexts, errors and the point queries. The rest of the ABI sits with its subject:
// ngp_model.cpp, ngp_snapshot.cpp, ngp_dataset.cpp, ngp_render.cpp, ngp_mesh.cpp, ngp_irradiance.cpp, ngp_train.cpp, ngp_multi.cpp, ngp_mc.cpp.
// Host logic only; every device computation lives in the .hip files. There is no CPU fallback: each entry point
// that computes needs a HIP device and fails with an error otherwise.
#include "ngp_host.h"

#include <cstdio>

using namespace ngp;

// ================================================================================================== C ABI
extern "C" {

const char* ngp_version(void) { return "ngp_hip 0.1 (gfx950)"; }

// NGP_TUNE goes through the same gate as ngp_set_schedule, on every kind of context: a refused list fails the creation, with the gate's message
static bool schedule_from_env_or_report(ngp_ctx* ctx) {
	try {
		schedule_from_env(ctx);
	} catch (const std::exception& e) {
		fprintf(stderr, "ngp_create: NGP_TUNE: %s\n", e.what());
		return false;
	}
	return true;
}

ngp_ctx* ngp_create(int device) {
	if (device == -1) { // host-only context: file formats and validation, no rendering (there is no CPU renderer)
		std::unique_ptr<ngp_ctx> ctx(new ngp_ctx());
		ctx->device = -1;
		return schedule_from_env_or_report(ctx.get()) ? ctx.release() : nullptr;
	}
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return nullptr;
	if (hipSetDevice(device) != hipSuccess) return nullptr;
	std::unique_ptr<ngp_ctx> ctx(new ngp_ctx());
	ctx->device = device;
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->n_cus = prop.multiProcessorCount;
	try {
		ctx->stream = new_stream();
	} catch (const std::exception&) {
		return nullptr;
	}
	return schedule_from_env_or_report(ctx.get()) ? ctx.release() : nullptr;
}

// peers first; then every owner of the context releases its resources on the owning device, after the last frame
void ngp_destroy(ngp_ctx* ctx) {
	if (!ctx) return;
	for (ngp_ctx* p : ctx->peers) ngp_destroy(p);
	ctx->peers.clear();
	if (ctx->device >= 0) {
		(void)hipSetDevice(ctx->device);
		if (ctx->last_stream) (void)hipStreamSynchronize(ctx->last_stream);
		free_model(ctx);
	}
	delete ctx;
}

const char* ngp_last_error(const ngp_ctx* ctx) { return ctx ? ctx->error.c_str() : "no HIP device / invalid context"; }

int ngp_grid_encode(ngp_ctx* ctx, uint32_t n, const float* pos01, uint16_t* out_fp16) {
	return guarded(ctx, [&] {
		require_model(ctx);
		ngp::sync_inference_model(ctx);
		if (n == 0) return;
		if (!pos01 || !out_fp16) throw std::runtime_error("null argument");
		DevArray<float> d_pos;
		d_pos.upload(pos01, (size_t)n * 3);
		const size_t width = ctx->M.wide.width ? ctx->M.wide.enc_dims : 32; // the position encoding's (padded) width
		DevArray<uint16_t> d_out((size_t)n * width);
		if (ctx->M.wide.width) launch_frequency_encode(ctx->M, n, d_pos.get(), d_out.get(), ctx->stream);
		else launch_grid_encode(ctx->M, n, d_pos.get(), d_out.get(), ctx->stream);
		NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
		NGP_HIP_CHECK(hipMemcpy(out_fp16, d_out.get(), d_out.bytes(), hipMemcpyDeviceToHost));
		NGP_HIP_CHECK(hipGetLastError());
	});
}

int ngp_density_gradient(ngp_ctx* ctx, uint32_t n, const float* pos01, float* out_grad) {
	return guarded(ctx, [&] {
		require_model(ctx);
		if (ctx->M.wide.width && (!ctx->M.wide.layers_t[0].n_mtiles || ctx->M.wide.enc_dims > ctx->M.wide.width))
			throw std::runtime_error("the density gradient of a Frequency / Identity-encoding model: implemented for up to 8 hidden density layers and an encoding no wider than the network");
		ngp::sync_inference_model(ctx);
		if (n == 0) return;
		if (!pos01 || !out_grad) throw std::runtime_error("null argument");
		DevArray<float> d_pos, d_out((size_t)n * 3);
		d_pos.upload(pos01, (size_t)n * 3);
		if (ctx->M.wide.width) launch_density_gradient_wide(ctx->M, n, d_pos.get(), d_out.get(), ctx->n_cus, ctx->stream);
		else launch_density_gradient(ctx->M, n, d_pos.get(), d_out.get(), ctx->stream);
		NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
		NGP_HIP_CHECK(hipMemcpy(out_grad, d_out.get(), d_out.bytes(), hipMemcpyDeviceToHost));
		NGP_HIP_CHECK(hipGetLastError());
	});
}

int ngp_network_inference(ngp_ctx* ctx, uint32_t n, const float* pos01, const float* dir01, uint16_t* out_fp16) {
	return guarded(ctx, [&] {
		require_model(ctx);
		ngp::sync_inference_model(ctx);
		if (n == 0) return;
		if (!pos01 || !dir01 || !out_fp16) throw std::runtime_error("null argument");
		DevArray<float> d_pos, d_dir;
		DevArray<uint16_t> d_out((size_t)n * 4);
		d_pos.upload(pos01, (size_t)n * 3);
		d_dir.upload(dir01, (size_t)n * 3);
		if (ctx->M.wide.width) launch_network_inference_wide(ctx->M, n, d_pos.get(), d_dir.get(), d_out.get(), ctx->n_cus, ctx->stream);
		else launch_network_inference(ctx->M, n, d_pos.get(), d_dir.get(), d_out.get(), ctx->stream);
		NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
		NGP_HIP_CHECK(hipMemcpy(out_fp16, d_out.get(), d_out.bytes(), hipMemcpyDeviceToHost));
		NGP_HIP_CHECK(hipGetLastError());
	});
}

int ngp_get_density_bitfield(ngp_ctx* ctx, uint8_t* out, float* out_mean) {
	return guarded(ctx, [&] {
		require_model(ctx);
		ngp::sync_inference_model(ctx);
		if (out) NGP_HIP_CHECK(hipMemcpy(out, ctx->d_bitfield.get(), (size_t)NERF_GRID_N_CELLS / 8 * NERF_CASCADES, hipMemcpyDeviceToHost));
		if (out_mean) *out_mean = ctx->bitfield_mean;
	});
}

int ngp_init_rays(ngp_ctx* ctx, const ngp_camera* cam, void* payloads_out) {
	return guarded(ctx, [&] {
		require_model(ctx);
		ngp::sync_inference_model(ctx);
		if (!cam || !payloads_out) throw std::runtime_error("null argument");
		DevArray<NerfPayload> d_p((size_t)cam->width * cam->height);
		CameraParams C = make_camera_params(*cam, cam->spp_index);
		launch_init_rays(ctx->M, C, d_p.get(), ctx->stream);
		NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
		NGP_HIP_CHECK(hipMemcpy(payloads_out, d_p.get(), d_p.bytes(), hipMemcpyDeviceToHost));
		NGP_HIP_CHECK(hipGetLastError());
	});
}

} // extern "C"
