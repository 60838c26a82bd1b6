// pybind11 module `pyngp`: the subset of the reference's src/python_api.cu that scripts/run.py's training, evaluation,
// screenshot and camera-path rendering paths use (Testbed, TestbedMode, RenderMode, LossType; load_*, train / frame,
// render, camera and render-state properties), bound to the C-ABI-backed ngp::Testbed shim. Same names and defaults
// as python_api.cu:263-733.
#include "testbed_shim.h"

#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

namespace py = pybind11;
using namespace ngp;

static std::array<float, 12> to_colmajor(const py::array_t<float, py::array::c_style | py::array::forcecast>& a) {
	if (a.ndim() != 2 || a.shape(0) != 3 || a.shape(1) != 4) throw std::runtime_error("expected a 3x4 matrix");
	std::array<float, 12> m;
	auto r = a.unchecked<2>();
	for (int c = 0; c < 4; ++c)
		for (int row = 0; row < 3; ++row) m[c * 3 + row] = r(row, c);
	return m;
}
static py::array_t<float> from_colmajor(const std::array<float, 12>& m) {
	py::array_t<float> a({3, 4});
	auto w = a.mutable_unchecked<2>();
	for (int c = 0; c < 4; ++c)
		for (int row = 0; row < 3; ++row) w(row, c) = m[c * 3 + row];
	return a;
}

// a bounding box argument: None, or (min3, max3) as any sequence of 6 floats / 2 x 3 array
static std::vector<float> aabb6_arg(const py::object& o) {
	if (o.is_none()) return {};
	py::array_t<float, py::array::c_style | py::array::forcecast> a = py::array_t<float, py::array::c_style | py::array::forcecast>::ensure(o);
	if (!a || a.size() != 6) throw std::runtime_error("aabb: None or (min xyz, max xyz)");
	return std::vector<float>(a.data(), a.data() + 6);
}

PYBIND11_MODULE(pyngp, m) {
	m.doc() = "MI355X-native NeRF renderer and trainer behind the instant-ngp Testbed API";
	py::enum_<ETestbedMode>(m, "TestbedMode")
		.value("Nerf", ETestbedMode::Nerf).value("Sdf", ETestbedMode::Sdf).value("Image", ETestbedMode::Image)
		.value("Volume", ETestbedMode::Volume).value("Geometry", ETestbedMode::Geometry).value("None", ETestbedMode::None)
		.export_values();
	// the reference registers the name "Shade" twice (python_api.cu:284-294), which pybind11 rejects at import;
	// ShadeNerf keeps its own name here
	py::enum_<EColorSpace>(m, "ColorSpace").value("Linear", EColorSpace::Linear).value("SRGB", EColorSpace::SRGB).value("VisPosNeg", EColorSpace::VisPosNeg).export_values();
	py::enum_<ELossType>(m, "LossType")
		.value("L2", ELossType::L2).value("L1", ELossType::L1).value("Mape", ELossType::Mape).value("Smape", ELossType::Smape)
		.value("Huber", ELossType::Huber).value("LogL1", ELossType::LogL1).value("RelativeL2", ELossType::RelativeL2)
		.export_values();
	py::enum_<ERenderMode>(m, "RenderMode")
		.value("AO", ERenderMode::AO).value("Shade", ERenderMode::Shade).value("Normals", ERenderMode::Normals)
		.value("Positions", ERenderMode::Positions).value("Depth", ERenderMode::Depth).value("Distortion", ERenderMode::Distortion)
		.value("Cost", ERenderMode::Cost).value("Slice", ERenderMode::Slice).value("ShadeNerf", ERenderMode::ShadeNerf)
		.value("ShadeEnvMap", ERenderMode::ShadeEnvMap).value("ShadeGridEnvMap", ERenderMode::ShadeGridEnvMap).value("ShadeIrradianceVolume", ERenderMode::ShadeIrradianceVolume)
		.export_values();

	// nested under Testbed like python_api.cu does (py::class_<Testbed::Nerf> nerf(testbed, "Nerf")): the exported enum
	// value TestbedMode.Nerf already owns the module-level name "Nerf"
	py::class_<Testbed> testbed(m, "Testbed");
	py::class_<Testbed::TrainingImageMetadata>(testbed, "TrainingImageMetadata")
		.def_readonly("resolution", &Testbed::TrainingImageMetadata::resolution)
		.def_readonly("focal_length", &Testbed::TrainingImageMetadata::focal_length)
		.def_readonly("principal_point", &Testbed::TrainingImageMetadata::principal_point);
	py::class_<Testbed::NerfDatasetView>(testbed, "NerfDataset")
		.def_readonly("n_images", &Testbed::NerfDatasetView::n_images)
		.def_readonly("metadata", &Testbed::NerfDatasetView::metadata)
		.def_readonly("aabb_scale", &Testbed::NerfDatasetView::aabb_scale)
		.def_readonly("scale", &Testbed::NerfDatasetView::scale)
		.def_readonly("offset", &Testbed::NerfDatasetView::offset);
	py::class_<Testbed::Nerf::Training>(testbed, "NerfTraining")
		.def_readonly("dataset", &Testbed::Nerf::Training::dataset)
		.def_readwrite("view", &Testbed::Nerf::Training::view)
		.def_readwrite("random_bg_color", &Testbed::Nerf::Training::random_bg_color)
		.def_readwrite("linear_colors", &Testbed::Nerf::Training::linear_colors)
		.def_readwrite("loss_type", &Testbed::Nerf::Training::loss_type)
		.def_readwrite("snap_to_pixel_centers", &Testbed::Nerf::Training::snap_to_pixel_centers)
		.def_readwrite("density_grid_decay", &Testbed::Nerf::Training::density_grid_decay)
		.def_readonly("n_images_for_training", &Testbed::Nerf::Training::n_images_for_training)
		.def_readwrite("near_distance", &Testbed::Nerf::Training::near_distance);
	py::class_<Testbed::Nerf>(testbed, "Nerf")
		.def_readwrite("render_min_transmittance", &Testbed::Nerf::render_min_transmittance)
		.def_readwrite("cone_angle_constant", &Testbed::Nerf::cone_angle_constant)
		.def_readwrite("sharpen", &Testbed::Nerf::sharpen)
		.def_readwrite("render_with_lens_distortion", &Testbed::Nerf::render_with_lens_distortion)
		.def_readonly("training", &Testbed::Nerf::training);
	py::class_<Testbed::BRDFParams>(testbed, "BRDFParams")
		.def(py::init<>()) // (a material for set_mesh_material: the defaults of testbed.brdf)
		.def_readwrite("metallic", &Testbed::BRDFParams::metallic).def_readwrite("subsurface", &Testbed::BRDFParams::subsurface)
		.def_readwrite("specular", &Testbed::BRDFParams::specular).def_readwrite("roughness", &Testbed::BRDFParams::roughness)
		.def_readwrite("sheen", &Testbed::BRDFParams::sheen).def_readwrite("clearcoat", &Testbed::BRDFParams::clearcoat)
		.def_readwrite("clearcoat_gloss", &Testbed::BRDFParams::clearcoat_gloss)
		.def_readwrite("basecolor", &Testbed::BRDFParams::basecolor).def_readwrite("ambientcolor", &Testbed::BRDFParams::ambientcolor);

	testbed
		.def(py::init<ETestbedMode, int>(), py::arg("mode") = ETestbedMode::None, py::arg("device") = 0)
		.def(py::init<ETestbedMode, const std::string&, int>(), py::arg("mode"), py::arg("data_path"), py::arg("device") = 0)
		.def(py::init<ETestbedMode, const std::vector<int>&>(), py::arg("mode"), py::arg("devices"), "Several GPUs behind one Testbed: the camera's tiles are dealt to all of them (devices[0] assembles the frame)")
		.def_property_readonly("n_devices", &Testbed::n_devices)
		.def("load_training_data", &Testbed::load_training_data, py::call_guard<py::gil_scoped_release>(), "Load training data from a given path.")
		.def("load_snapshot", &Testbed::load_snapshot, py::arg("path"), "Load a previously saved snapshot")
		.def("save_snapshot", &Testbed::save_snapshot, py::arg("path"), py::arg("include_optimizer_state") = false, py::arg("compress") = true)
		.def("load_file", &Testbed::load_file, py::arg("path"))
		.def("load_mesh", &Testbed::load_mesh, py::arg("path"), py::arg("center") = std::array<float, 3>{0.f, 0.f, 0.f})
		.def("reset_camera", &Testbed::reset_camera)
		.def("set_nerf_camera_matrix", [](Testbed& t, const py::array_t<float, py::array::c_style | py::array::forcecast>& a) { t.set_nerf_camera_matrix(to_colmajor(a)); })
		.def("set_camera_to_training_view", &Testbed::set_camera_to_training_view)
		.def("compute_envmap", &Testbed::computeEnvmapMultipleMain, py::arg("n_theta") = 256, py::arg("n_phi") = 128, py::arg("n_origin") = 1)
		.def("compute_envmap_grid", &Testbed::computeEnvmapGrid, py::arg("grid_x") = 8, py::arg("grid_y") = 8, py::arg("n_theta") = 64, py::arg("n_phi") = 32, py::arg("shell_radius") = 1.0f)
		.def("render", [](Testbed& t, int width, int height, int spp, bool linear, float start_t, float end_t, float fps, float shutter_fraction) {
				// a fresh array per call, like python_api.cu:124-202 -- whose memory is page-locked and pooled (ngp_host_alloc), so the
				// device-to-host copy is a single DMA; the array owns its buffer and returns it to the pool when collected
				const size_t bytes = (size_t)height * width * 4 * sizeof(float);
				float* mem = (float*)ngp_host_alloc(bytes);
				if (!mem) throw std::runtime_error("out of host memory");
				py::capsule owner(mem, [](void* p) { ngp_host_free(p); });
				py::array_t<float> result({(py::ssize_t)height, (py::ssize_t)width, (py::ssize_t)4}, mem, owner);
				{
					py::gil_scoped_release release;
					t.render_to_cpu(result.mutable_data(), width, height, spp, linear, start_t, end_t, fps, shutter_fraction);
				}
				return result;
			}, "Renders an image at the requested resolution. Does not require a window.",
			py::arg("width") = 1920, py::arg("height") = 1080, py::arg("spp") = 1, py::arg("linear") = true, py::arg("start_t") = -1.f,
			py::arg("end_t") = -1.f, py::arg("fps") = 30.f, py::arg("shutter_fraction") = 1.0f)
		.def_property("camera_matrix", [](Testbed& t) { return from_colmajor(t.m_camera); },
			[](Testbed& t, const py::array_t<float, py::array::c_style | py::array::forcecast>& a) { t.m_camera = to_colmajor(a); })
		.def_property("fov", &Testbed::fov, &Testbed::set_fov)
		.def_readwrite("fov_axis", &Testbed::m_fov_axis)
		.def_readwrite("relative_focal_length", &Testbed::m_relative_focal_length)
		.def_readwrite("screen_center", &Testbed::m_screen_center)
		.def_readwrite("zoom", &Testbed::m_zoom)
		.def_readwrite("scale", &Testbed::m_scale)
		.def_readwrite("background_color", &Testbed::m_background_color)
		.def_readwrite("snap_to_pixel_centers", &Testbed::m_snap_to_pixel_centers)
		.def_readwrite("exposure", &Testbed::m_exposure)
		.def_readwrite("render_mode", &Testbed::m_render_mode)
		.def_readwrite("color_space", &Testbed::m_color_space)
		.def_readwrite("aperture_size", &Testbed::m_aperture_size)
		.def_readwrite("slice_plane_z", &Testbed::m_slice_plane_z)
		.def_readwrite("render_ground_truth", &Testbed::m_render_ground_truth)
		.def_readwrite("render_near_distance", &Testbed::m_render_near_distance)
		.def_readwrite("sun_dir", &Testbed::m_sun_dir)
		.def_readwrite("up_dir", &Testbed::m_up_dir)
		.def_readwrite("root_dir", &Testbed::m_root_dir)
		.def_readonly("data_path", &Testbed::m_data_path)
		.def_readonly("aabb", &Testbed::m_aabb)
		.def_property("render_aabb", [](Testbed& t) { return t.m_render_aabb; }, &Testbed::set_render_aabb, "crop box of the render: [min xyz, max xyz] in ngp space")
		.def_readonly("mode", &Testbed::m_testbed_mode)
		.def_readonly("training_step", &Testbed::m_training_step)
		.def_readonly("loss", &Testbed::m_loss)
		.def_readwrite("brdf", &Testbed::brdf)
		.def_readwrite("shall_train", &Testbed::m_train)
		.def_readwrite("shall_train_encoding", &Testbed::m_train_encoding)
		.def_readwrite("shall_train_network", &Testbed::m_train_network)
		.def_readwrite("training_batch_size", &Testbed::m_training_batch_size)
		.def_readwrite("seed", &Testbed::m_seed)
		.def("want_repl", [](Testbed&) { return false; }, "scripts/run.py polls this inside its training loop (the GUI's console key); headless: never")
		.def("init_window", [](Testbed&, int, int, bool, bool) { throw std::runtime_error("this build is headless: render() / frame() work without a window"); },
			py::arg("width"), py::arg("height"), py::arg("hidden") = false, py::arg("second_window") = false)
		.def("init_vr", [](Testbed&) { throw std::runtime_error("this build is headless: no VR"); })
		.def("load_camera_path", &Testbed::load_camera_path, py::arg("path"), "Load a camera path")
		.def("set_camera_from_time", &Testbed::set_camera_from_time, py::arg("t"), "place the camera on the loaded path, t in [0, 1]")
		.def_readwrite("camera_smoothing", &Testbed::m_camera_smoothing)
		.def("compute_marching_cubes_mesh", [](Testbed& t, const std::array<uint32_t, 3>& res, py::object aabb, float thresh) {
			const std::vector<float> box = aabb6_arg(aabb);
			Testbed::MarchingCubesMesh m;
			{
				py::gil_scoped_release nogil;
				m = t.compute_marching_cubes_mesh(res, box.empty() ? nullptr : box.data(), thresh);
			}
			auto rows = [](const auto& v) {
				using T = typename std::decay_t<decltype(v)>::value_type;
				py::array_t<T> a({(py::ssize_t)(v.size() / 3), (py::ssize_t)3});
				if (!v.empty()) memcpy(a.mutable_data(), v.data(), v.size() * sizeof(T));
				return a;
			};
			py::dict d;
			d["V"] = rows(m.V); d["N"] = rows(m.N); d["C"] = rows(m.C); d["F"] = rows(m.F);
			return d;
		}, py::arg("resolution") = std::array<uint32_t, 3>{256, 256, 256}, py::arg("aabb") = py::none(), py::arg("thresh") = 2.5f,
		   "Marching cubes of the density: {'V', 'N', 'C', 'F'} in ngp space (aabb: None = the render aabb, or (min, max))")
		.def("compute_and_save_marching_cubes_mesh", [](Testbed& t, const std::string& filename, const std::array<uint32_t, 3>& res, py::object aabb, float thresh, bool uvs) {
			const std::vector<float> box = aabb6_arg(aabb);
			py::gil_scoped_release nogil;
			t.compute_and_save_marching_cubes_mesh(filename, res, box.empty() ? nullptr : box.data(), thresh, uvs);
		}, py::arg("filename"), py::arg("resolution") = std::array<uint32_t, 3>{256, 256, 256}, py::arg("aabb") = py::none(), py::arg("thresh") = 2.5f,
		   py::arg("generate_uvs_for_obj_file") = false, "Marching cubes of the density, saved as .obj or .ply in dataset space")
		.def("compute_irradiance_at_points", [](Testbed& t, py::array_t<float, py::array::c_style | py::array::forcecast> positions,
		                                        py::array_t<float, py::array::c_style | py::array::forcecast> normals, uint32_t n_u, uint32_t n_v, float offset,
		                                        bool occlude_by_meshes) {
			if (positions.ndim() != 2 || positions.shape(1) != 3 || normals.ndim() != 2 || normals.shape(1) != 3 || positions.shape(0) != normals.shape(0))
				throw std::runtime_error("positions and normals: (n, 3) each");
			const uint32_t n = (uint32_t)positions.shape(0);
			std::vector<float> e;
			{
				py::gil_scoped_release nogil;
				e = t.compute_irradiance_at_points(positions.data(), normals.data(), n, n_u, n_v, offset, occlude_by_meshes);
			}
			py::array_t<float> a({(py::ssize_t)n, (py::ssize_t)4});
			if (n) memcpy(a.mutable_data(), e.data(), e.size() * sizeof(float));
			return a;
		}, py::arg("positions"), py::arg("normals"), py::arg("n_u") = 16, py::arg("n_v") = 16, py::arg("offset") = 1e-4f, py::arg("occlude_by_meshes") = true,
		   "This project's own: the irradiance traced at surface points through the NeRF, (n, 4) = rgb, fraction of rays no mesh blocks")
		.def("compute_irradiance_sh_at_points", [](Testbed& t, py::array_t<float, py::array::c_style | py::array::forcecast> positions, uint32_t n_u, uint32_t n_v,
		                                           bool occlude_by_meshes) {
			if (positions.ndim() != 2 || positions.shape(1) != 3) throw std::runtime_error("positions: (n, 3)");
			const uint32_t n = (uint32_t)positions.shape(0);
			std::vector<float> sh;
			{
				py::gil_scoped_release nogil;
				sh = t.compute_irradiance_sh_at_points(positions.data(), n, n_u, n_v, occlude_by_meshes);
			}
			py::array_t<float> a({(py::ssize_t)n, (py::ssize_t)28});
			if (n) memcpy(a.mutable_data(), sh.data(), sh.size() * sizeof(float));
			return a;
		}, py::arg("positions"), py::arg("n_u") = 32, py::arg("n_v") = 32, py::arg("occlude_by_meshes") = true,
		   "This project's own: SH9 irradiance probes traced at the points, (n, 28) = 9 coefficients x rgb, fraction of rays no mesh blocks")
		.def("compute_irradiance_volume", [](Testbed& t, const std::array<uint32_t, 3>& res, py::object aabb, uint32_t n_u, uint32_t n_v, bool occlude_by_meshes, uint32_t bounces,
		                                     py::object albedo, bool sun, bool sun_nerf_shadow) {
			const std::vector<float> box = aabb6_arg(aabb);
			const bool own_albedo = !albedo.is_none();
			const std::array<float, 3> al = own_albedo ? albedo.cast<std::array<float, 3>>() : std::array<float, 3>{};
			std::vector<float> sh;
			std::array<float, 6> used{};
			{
				py::gil_scoped_release nogil;
				sh = t.compute_irradiance_volume(res, box.empty() ? nullptr : box.data(), n_u, n_v, occlude_by_meshes, used.data(), bounces, own_albedo ? al.data() : nullptr, false, sun, sun_nerf_shadow);
			}
			py::array_t<float> a({(py::ssize_t)res[2], (py::ssize_t)res[1], (py::ssize_t)res[0], (py::ssize_t)28});
			if (!sh.empty()) memcpy(a.mutable_data(), sh.data(), sh.size() * sizeof(float));
			py::dict d;
			d["sh"] = a;
			d["aabb"] = py::make_tuple(std::array<float, 3>{used[0], used[1], used[2]}, std::array<float, 3>{used[3], used[4], used[5]});
			return d;
		}, py::arg("resolution"), py::arg("aabb") = py::none(), py::arg("n_u") = 32, py::arg("n_v") = 32, py::arg("occlude_by_meshes") = true, py::arg("bounces") = 0,
		   py::arg("albedo") = py::none(), py::arg("sun") = false, py::arg("sun_nerf_shadow") = false,
		   "This project's own: a lattice of SH9 irradiance probes, traced and kept for irradiance_volume_lookup: {'sh': (rz, ry, rx, 28), 'aabb': (min, max)} "
		   "(aabb: None = the render aabb, or (min, max); bounces: passes of diffuse interreflection off the meshes, of colour albedo = (r, g, b) in [0, 1], None = the base colour squared; "
		   "sun: the frame's sun, sun_dir with irradiance_volume_sun_radiance, throws its first bounce off the meshes into the records ahead of the passes; "
		   "sun_nerf_shadow: with sun, the NeRF's density stands in front of it, traced with render_min_transmittance)")
		.def("get_irradiance_volume", [](Testbed& t) {
			std::array<uint32_t, 3> res{};
			std::array<float, 6> box{};
			std::vector<float> sh;
			{
				py::gil_scoped_release nogil;
				sh = t.get_irradiance_volume(res, box.data());
			}
			py::array_t<float> a({(py::ssize_t)res[2], (py::ssize_t)res[1], (py::ssize_t)res[0], (py::ssize_t)28});
			if (!sh.empty()) memcpy(a.mutable_data(), sh.data(), sh.size() * sizeof(float));
			py::dict d;
			d["sh"] = a;
			d["aabb"] = py::make_tuple(std::array<float, 3>{box[0], box[1], box[2]}, std::array<float, 3>{box[3], box[4], box[5]});
			return d;
		}, "The irradiance volume the context holds, as compute_irradiance_volume returns it (a ShadeIrradianceVolume render computes a default one when there is none)")
		.def_readwrite("irradiance_volume_bounces", &Testbed::m_irradiance_volume_bounces,
		               "passes of diffuse interreflection off the meshes in the volume a ShadeIrradianceVolume render computes when the context holds none (albedo: the base colour squared)")
		.def_readwrite("irradiance_volume_sun", &Testbed::m_irradiance_volume_sun,
		               "the volume a ShadeIrradianceVolume render computes when the context holds none also holds the sun's first bounce off the meshes (sun_dir, irradiance_volume_sun_radiance)")
		.def_readwrite("sun_nerf_shadow", &Testbed::m_sun_nerf_shadow,
		               "Geometry frames with meshes and a model: the NeRF's density shadows the frames' own sun on mesh pixels (default False)")
		.def_readwrite("sun_nerf_shadow_min_transmittance", &Testbed::m_sun_nerf_shadow_min_transmittance, "with sun_nerf_shadow: the shadow rays' transmittance floor (0.01)")
		.def_readwrite("sun_nerf_shadow_t_min", &Testbed::m_sun_nerf_shadow_t_min, "with sun_nerf_shadow: the NeRF is ignored within this distance of the surface (0)")
		.def_readwrite("sun_disk", &Testbed::m_sun_disk,
		               "Geometry frames with meshes: the sun has a disk, sun_disk_rays shadow rays a pixel against all meshes give soft shadows on mesh pixels and, with mesh_shadow_on_nerf, on NeRF pixels (default False)")
		.def_readwrite("sun_disk_angular_radius", &Testbed::m_sun_disk_angular_radius, "with sun_disk: the disk's angular radius in rad, at most 0.5 (0.00465, the real sun)")
		.def_readwrite("sun_disk_rays", &Testbed::m_sun_disk_rays, "with sun_disk: shadow rays a pixel, 1, 2, 4, 8 or 16 (16)")
		.def_readwrite("mesh_shadow_on_nerf", &Testbed::m_mesh_shadow_on_nerf,
		               "Geometry frames with meshes and a model: the meshes throw the sun's shadow onto the NeRF (default False)")
		.def_readwrite("mesh_shadow_on_nerf_strength", &Testbed::m_mesh_shadow_on_nerf_strength, "with mesh_shadow_on_nerf: the share of a shadowed NeRF pixel's colour the shadow takes away (0.5)")
		.def_readwrite("mesh_shadow_on_nerf_bias", &Testbed::m_mesh_shadow_on_nerf_bias, "with mesh_shadow_on_nerf: how far the shadow ray's origin is lifted off the NeRF's surface point towards the sun (1e-2)")
		.def_readwrite("ambient_change_on_nerf", &Testbed::m_ambient_change_on_nerf,
		               "Geometry frames with meshes and a model: every NeRF pixel that owns a surface point is scaled by E_after / E_before there, the irradiance volume "
		               "over the reference volume; a missing volume is computed before the frame (default False)")
		.def_readwrite("ambient_change_on_nerf_min_irradiance", &Testbed::m_ambient_change_on_nerf_min_irradiance, "with ambient_change_on_nerf: a channel whose reference irradiance is not above this keeps its colour (1e-3)")
		.def_readwrite("ambient_change_on_nerf_max_gain", &Testbed::m_ambient_change_on_nerf_max_gain, "with ambient_change_on_nerf: the cap on the ratio (4)")
		.def_readwrite("mesh_reflection", &Testbed::m_mesh_reflection,
		               "This project's own: Geometry frames with meshes and a model, the four shade modes: a mesh pixel whose primary ray found a triangle adds strength * F * (the NeRF's radiance along its mirror direction) (default False)")
		.def("set_mesh_material", &Testbed::set_mesh_material, py::arg("mesh"), py::arg("material"),
		     "Give an inserted mesh its own material (a BRDFParams); a mesh without one is shaded with testbed.brdf. Kept across load_training_data.")
		.def("clear_mesh_material", &Testbed::clear_mesh_material, py::arg("mesh"), "Shade the mesh with testbed.brdf again.")
		.def("mesh_material", [](Testbed& t, int mesh) -> py::object {
			Testbed::BRDFParams b;
			if (!t.mesh_material(mesh, b)) return py::none();
			return py::cast(b);
		}, py::arg("mesh"), "The mesh's own material (a BRDFParams), or None where it is shaded with testbed.brdf.")
		.def("set_mesh_albedo", &Testbed::set_mesh_albedo, py::arg("mesh"), py::arg("rgb"),
		     "Give an inserted mesh its own albedo in the SH9 volume's bounce and sun passes (three channels in [0, 1]); a mesh without one uses the computation's. Kept across load_training_data.")
		.def("clear_mesh_albedo", &Testbed::clear_mesh_albedo, py::arg("mesh"), "The mesh bounces light with the computation's albedo again.")
		.def("mesh_albedo", [](Testbed& t, int mesh) -> py::object {
			std::array<float, 3> a{};
			if (!t.mesh_albedo(mesh, a)) return py::none();
			return py::make_tuple(a[0], a[1], a[2]);
		}, py::arg("mesh"), "The mesh's own albedo (r, g, b), or None where the volume's passes use the computation's.")
		.def_readwrite("irradiance_volume_albedo_from_materials", &Testbed::m_irradiance_volume_albedo_from_materials,
		               "the volumes computed here (compute_irradiance_volume, the default volume of a render) take the albedo of a mesh that owns a material and no albedo from that material: the base colour squared (default False)")
		.def_readwrite("mesh_reflection_meshes", &Testbed::m_mesh_reflection_meshes,
		               "with mesh_reflection: a mirror ray that a mesh cuts carries that mesh's own shade at the hit, behind the NeRF along the ray (default False)")
		.def_readwrite("mesh_reflection_strength", &Testbed::m_mesh_reflection_strength, "with mesh_reflection: the factor on the reflected radiance (1)")
		.def_readwrite("mesh_reflection_min_transmittance", &Testbed::m_mesh_reflection_min_transmittance, "with mesh_reflection: the reflection rays' transmittance floor (0.01)")
		.def_readwrite("mesh_reflection_t_min", &Testbed::m_mesh_reflection_t_min, "with mesh_reflection: the NeRF is ignored within this distance of the surface (0)")
		.def("compute_reference_irradiance_volume", [](Testbed& t, const std::array<uint32_t, 3>& res, py::object aabb, uint32_t n_u, uint32_t n_v) {
			const std::vector<float> box = aabb6_arg(aabb);
			std::vector<float> sh;
			std::array<float, 6> used{};
			{
				py::gil_scoped_release nogil;
				sh = t.compute_reference_irradiance_volume(res, box.empty() ? nullptr : box.data(), n_u, n_v, used.data());
			}
			py::array_t<float> a({(py::ssize_t)res[2], (py::ssize_t)res[1], (py::ssize_t)res[0], (py::ssize_t)28});
			if (!sh.empty()) memcpy(a.mutable_data(), sh.data(), sh.size() * sizeof(float));
			py::dict d;
			d["sh"] = a;
			d["aabb"] = py::make_tuple(std::array<float, 3>{used[0], used[1], used[2]}, std::array<float, 3>{used[3], used[4], used[5]});
			return d;
		}, py::arg("resolution"), py::arg("aabb") = py::none(), py::arg("n_u") = 32, py::arg("n_v") = 32,
		   "This project's own: the reference volume of ambient_change_on_nerf, the scene before the meshes: the lattice of compute_irradiance_volume traced with the meshes "
		   "occluding nothing, kept beside the irradiance volume: {'sh': (rz, ry, rx, 28), 'aabb': (min, max)}")
		.def_readwrite("irradiance_volume_sun_nerf_shadow", &Testbed::m_irradiance_volume_sun_nerf_shadow,
		               "with irradiance_volume_sun: the NeRF's density shadows that sun in the default volume (render_min_transmittance, t_min 0)")
		.def_readwrite("irradiance_volume_sun_radiance", &Testbed::m_irradiance_volume_sun_radiance, "what a surface facing the sun receives in a sunlit volume; default: the frames' sun colour")
		.def_readwrite("irradiance_volume_res", &Testbed::m_irradiance_volume_res, "probes per axis of the volume a ShadeIrradianceVolume render computes when the context holds none")
		.def("irradiance_volume_lookup", [](Testbed& t, py::array_t<float, py::array::c_style | py::array::forcecast> positions,
		                                    py::array_t<float, py::array::c_style | py::array::forcecast> normals, bool visible) {
			if (positions.ndim() != 2 || positions.shape(1) != 3 || normals.ndim() != 2 || normals.shape(1) != 3 || positions.shape(0) != normals.shape(0))
				throw std::runtime_error("positions and normals: (n, 3) each");
			const uint32_t n = (uint32_t)positions.shape(0);
			std::vector<float> e;
			{
				py::gil_scoped_release nogil;
				e = t.irradiance_volume_lookup(positions.data(), normals.data(), n, visible);
			}
			py::array_t<float> a({(py::ssize_t)n, (py::ssize_t)4});
			if (n) memcpy(a.mutable_data(), e.data(), e.size() * sizeof(float));
			return a;
		}, py::arg("positions"), py::arg("normals"), py::arg("visible") = false,
		   "E(p, n) read from the irradiance volume: (n, 4) = rgb, weight of the live probes around the point (visible: weighted by the probes' visibility)")
		.def("compute_irradiance_volume_visibility", [](Testbed& t, uint32_t n_u, uint32_t n_v, uint32_t sharpness_log2, float max_distance, float normal_bias) {
			std::array<uint32_t, 3> res{};
			std::vector<float> maps;
			{
				py::gil_scoped_release nogil;
				maps = t.compute_irradiance_volume_visibility(n_u, n_v, sharpness_log2, max_distance, normal_bias, &res);
			}
			py::array_t<float> a({(py::ssize_t)res[2], (py::ssize_t)res[1], (py::ssize_t)res[0], (py::ssize_t)64, (py::ssize_t)2});
			if (!maps.empty()) memcpy(a.mutable_data(), maps.data(), maps.size() * sizeof(float));
			return a;
		}, py::arg("n_u") = 16, py::arg("n_v") = 16, py::arg("sharpness_log2") = 5, py::arg("max_distance") = 0.f, py::arg("normal_bias") = 0.f,
		   "This project's own: distance maps for the probes of the held irradiance volume, (rz, ry, rx, 64, 2) = mean and mean squared distance to the nearest mesh per "
		   "octahedral texel; while they are held, ShadeIrradianceVolume frames weight every probe by its visibility")
		.def_readwrite("irradiance_volume_visibility", &Testbed::m_irradiance_volume_visibility,
		               "the default volume a ShadeIrradianceVolume render computes also gets visibility (compute_irradiance_volume_visibility with its defaults)")
		.def("frame", &Testbed::frame, py::call_guard<py::gil_scoped_release>(), "Process a single frame: one training step when shall_train is set (headless, nothing is drawn).")
		.def("train", &Testbed::train, py::call_guard<py::gil_scoped_release>(), "Perform a single training step with a specified batch size.")
		.def("reset", &Testbed::reset_network, py::arg("reset_density_grid") = true, "Reset training.")
		.def("reload_network_from_file", &Testbed::reload_network_from_file, py::arg("path") = "", "Reload the network from a config file.")
		.def("set_training_image", [](Testbed& t, int frame_idx, py::array_t<float, py::array::c_style | py::array::forcecast> img) {
				py::buffer_info b = img.request();
				if (b.ndim != 3 || b.shape[2] != 4) throw std::runtime_error("image should be (H,W,C) where C=4");
				t.set_training_image(frame_idx, (int)b.shape[1], (int)b.shape[0], (const float*)b.ptr);
			}, py::arg("frame_idx"), py::arg("img"),
			"nerf.training.set_image of the reference (python_api.cu:691-697): a float (H,W,4) image, linear colour space, premultiplied alpha")
		.def_readonly("nerf", &Testbed::nerf);
}
