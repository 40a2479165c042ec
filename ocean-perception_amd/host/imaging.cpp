// imaging.cpp -- bm::imaging free functions over the C ABI (see imaging.hpp).
#include "imaging.hpp"

#include <cstdio>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>

namespace bm {
namespace imaging {
namespace {

int g_device = 0;
pm_handle* g_handle = nullptr;
std::mutex g_mutex;

// A failed call throws with the error text of the handle it ran on.
void CheckOn(pm_handle* h, int status, const char* what) {
  if (status == PM_OK) return;
  std::string msg = std::string(what) + ": " + pm_status_string(status);
  if (h) msg += std::string(" -- ") + pm_last_error(h);
  throw std::runtime_error(msg);
}

void Check(int status, const char* what) { CheckOn(g_handle, status, what); }  // the imaging context's calls

pm_handle* Context() {
  if (g_handle) return g_handle;
  pm_params p;
  pm_params_default(&p, PM_SEM_GPU);
  pm_handle* h = nullptr;
  const int rc = pm_create(&p, g_device, 16, 16, 1, &h);
  if (rc != PM_OK) {
    std::string msg = std::string("bm::imaging: pm_create: ") + pm_status_string(rc);
    if (h) msg += std::string(" -- ") + pm_last_error(h);
    pm_destroy(h);
    throw std::runtime_error(msg);
  }
  g_handle = h;
  return g_handle;
}

template <typename T>
size_t Bytes(const Image<T>& im) { return sizeof(T) * (size_t)im.rows * im.cols; }

// Any number of device buffers on one handle -- the imaging context's or a matcher's --, freed on every way out.  Check
// reports with that handle's error text.
class DeviceBuffers {
 public:
  explicit DeviceBuffers(pm_handle* h) : h_(h) {}
  ~DeviceBuffers() {
    for (void* q : p_) pm_device_free(h_, q);
  }
  DeviceBuffers(const DeviceBuffers&) = delete;
  DeviceBuffers& operator=(const DeviceBuffers&) = delete;
  pm_handle* handle() const { return h_; }
  void Check(int status, const char* what) const { CheckOn(h_, status, what); }
  template <typename T = void>
  T* Get(size_t bytes) {
    p_.push_back(nullptr);  // its place first: the buffer is owned from the moment it exists
    Check(pm_device_malloc(h_, bytes, &p_.back()), "pm_device_malloc");
    return static_cast<T*>(p_.back());
  }
  template <typename T>
  T* Put(const void* src, size_t bytes) {
    T* q = Get<T>(bytes);
    Check(pm_upload(h_, q, src, bytes), "pm_upload");
    return q;
  }
  // The download into an optional output image, which takes the result's size first.
  template <typename T>
  void Fetch(Image<T>* out, const void* d_src, int rows, int cols) const {
    if (out->rows != rows || out->cols != cols) out->create(rows, cols);
    Check(pm_download(h_, out->data(), d_src, Bytes(*out)), "pm_download");
  }

 private:
  pm_handle* h_;
  std::vector<void*> p_;
};

// One of them.
class DeviceBuffer : private DeviceBuffers {
 public:
  DeviceBuffer(pm_handle* h, size_t bytes) : DeviceBuffers(h), p_(Get(bytes)) {}
  template <typename T>
  T* as() { return static_cast<T*>(p_); }
  void Upload(const void* src, size_t bytes) { Check(pm_upload(handle(), p_, src, bytes), "pm_upload"); }
  void Download(void* dst, size_t bytes) { Check(pm_download(handle(), dst, p_, bytes), "pm_download"); }
  template <typename T>
  void DownloadInto(Image<T>* out, int rows, int cols) { Fetch(out, p_, rows, cols); }

 private:
  void* p_;
};

pm_motion ToC(const Motion& m) {
  pm_motion out;
  for (size_t i = 0; i < 9; ++i) out.R[i] = m.R[i];
  for (size_t i = 0; i < 3; ++i) out.t[i] = m.t[i];
  return out;
}

Motion FromC(const pm_motion& m) {
  Motion out;
  for (size_t i = 0; i < 9; ++i) out.R[i] = m.R[i];
  for (size_t i = 0; i < 3; ++i) out.t[i] = m.t[i];
  return out;
}

// The handle of the sequence stages: the matcher's, not the imaging context's.
pm_handle* MatcherHandle(pm::PatchmatchGpu& matcher, const char* who) {
  pm_handle* h = matcher.handle();
  if (!h) throw std::runtime_error(std::string(who) + ": the matcher has no handle yet (plan it or match once)");
  return h;
}

void SameSize(int r0, int c0, int r1, int c1, const char* what) {
  if (r0 != r1 || c0 != c1 || r0 <= 0 || c0 <= 0) throw std::invalid_argument(std::string(what) + ": image sizes differ or are empty");
}

}  // namespace

void SetDevice(int device) {
  std::lock_guard<std::mutex> lock(g_mutex);
  if (g_handle && device != g_device) {
    pm_destroy(g_handle);
    g_handle = nullptr;
  }
  g_device = device;
}

Image3f CastImage3bTo3f(const Image3b& im) {
  Image3f out(im.rows, im.cols);
  const float s = (float)(1.0 / 255.0);  // kUint8ToFloat, image_util.cpp:10
  for (int y = 0; y < im.rows; ++y)
    for (int x = 0; x < im.cols; ++x)
      for (int c = 0; c < 3; ++c) out.at(y, x).v[c] = (float)im.at(y, x).v[c] * s;
  return out;
}

Image1f ComputeIntensity(const Image3f& bgr) {
  std::lock_guard<std::mutex> lock(g_mutex);
  pm_handle* h = Context();
  DeviceBuffer d_in(h, Bytes(bgr)), d_out(h, sizeof(float) * (size_t)bgr.rows * bgr.cols);
  d_in.Upload(bgr.data(), Bytes(bgr));
  Check(pm_compute_intensity(h, d_in.as<float>(), bgr.rows, bgr.cols, d_out.as<float>()), "pm_compute_intensity");
  Image1f out(bgr.rows, bgr.cols);
  d_out.Download(out.data(), Bytes(out));
  return out;
}

Image3f EstimateIlluminantGaussian(const Image3f& bgr, int ksizeX, int ksizeY, double sigmaX, double sigmaY) {
  if (ksizeX != ksizeY || sigmaX != sigmaY)
    throw std::invalid_argument("EstimateIlluminantGaussian: only square kernels (the reference's only use)");
  std::lock_guard<std::mutex> lock(g_mutex);
  pm_handle* h = Context();
  DeviceBuffer d_in(h, Bytes(bgr)), d_out(h, Bytes(bgr));
  d_in.Upload(bgr.data(), Bytes(bgr));
  Check(pm_gaussian_blur(h, d_in.as<float>(), bgr.rows, bgr.cols, 3, ksizeX, sigmaX, d_out.as<float>()),
        "pm_gaussian_blur");
  Image3f out(bgr.rows, bgr.cols);
  d_out.Download(out.data(), Bytes(out));
  // Akkaynak et al. multiply by a factor of 2 to get the illuminant map (illuminant.cpp:19-20); exact in float
  for (int y = 0; y < out.rows; ++y)
    for (int x = 0; x < out.cols; ++x)
      for (int c = 0; c < 3; ++c) out.at(y, x).v[c] *= 2.0f;
  return out;
}

namespace {
template <typename T>
Image<T> GuidedFilter(const Image1f& guide, const Image<T>& src, int channels, int r, double eps, int s, float scale) {
  SameSize(guide.rows, guide.cols, src.rows, src.cols, "fastGuidedFilter");
  std::lock_guard<std::mutex> lock(g_mutex);
  pm_handle* h = Context();
  DeviceBuffer d_g(h, Bytes(guide)), d_p(h, Bytes(src));
  d_g.Upload(guide.data(), Bytes(guide));
  d_p.Upload(src.data(), Bytes(src));
  Check(pm_fast_guided_filter(h, d_g.as<float>(), d_p.as<float>(), src.rows, src.cols, channels, r, eps, s, scale,
                              d_p.as<float>()),
        "pm_fast_guided_filter");
  Image<T> out(src.rows, src.cols);
  d_p.Download(out.data(), Bytes(out));
  return out;
}
}  // namespace

Image1f fastGuidedFilter(const Image1f& guide, const Image1f& src, int r, double eps, int s) {
  return GuidedFilter(guide, src, 1, r, eps, s, 1.0f);
}

Image3f fastGuidedFilter(const Image1f& guide, const Image3f& src, int r, double eps, int s) {
  return GuidedFilter(guide, src, 3, r, eps, s, 1.0f);
}

Image3f EstimateIlluminantRangeGuided(const Image3f& bgr, const Image1f& range, int r, double eps, int s) {
  // Akkaynak et al. multiply by a factor of 2 to get the illuminant map (illuminant.cpp:31-33): the kernel's scale
  return GuidedFilter(range, bgr, 3, r, eps, s, 2.0f);
}

Image3f Normalize(const Image3f& bgr) {
  std::lock_guard<std::mutex> lock(g_mutex);
  pm_handle* h = Context();
  DeviceBuffer d_in(h, Bytes(bgr)), d_out(h, Bytes(bgr));
  d_in.Upload(bgr.data(), Bytes(bgr));
  Check(pm_normalize(h, d_in.as<float>(), bgr.rows, bgr.cols, d_out.as<float>()), "pm_normalize");
  Image3f out(bgr.rows, bgr.cols);
  d_out.Download(out.data(), Bytes(out));
  return out;
}

Image3f NormalizeColorIlluminant(const Image3f bgr) {
  std::lock_guard<std::mutex> lock(g_mutex);
  pm_handle* h = Context();
  DeviceBuffer d_in(h, Bytes(bgr)), d_out(h, Bytes(bgr));
  d_in.Upload(bgr.data(), Bytes(bgr));
  Check(pm_normalize_color_illuminant(h, d_in.as<float>(), bgr.rows, bgr.cols, d_out.as<float>()),
        "pm_normalize_color_illuminant");
  Image3f out(bgr.rows, bgr.cols);
  d_out.Download(out.data(), Bytes(out));
  return out;
}

float FindDarkFast(const Image1f& intensity, const Image1f& range, float percentile, Image1b& mask) {
  SameSize(intensity.rows, intensity.cols, range.rows, range.cols, "FindDarkFast");
  std::lock_guard<std::mutex> lock(g_mutex);
  pm_handle* h = Context();
  DeviceBuffer d_i(h, Bytes(intensity)), d_r(h, Bytes(range)), d_m(h, (size_t)intensity.rows * intensity.cols);
  d_i.Upload(intensity.data(), Bytes(intensity));
  d_r.Upload(range.data(), Bytes(range));
  float thr = 0.f;
  Check(pm_find_dark(h, d_i.as<float>(), d_r.as<float>(), intensity.rows, intensity.cols, percentile,
                     d_m.as<uint8_t>(), &thr),
        "pm_find_dark");
  d_m.DownloadInto(&mask, intensity.rows, intensity.cols);
  return thr;
}

Image3f RemoveBackscatter(const Image3f& bgr, const Image1f& range, const Vector3f& B, const Vector3f& beta_B) {
  SameSize(bgr.rows, bgr.cols, range.rows, range.cols, "RemoveBackscatter");
  std::lock_guard<std::mutex> lock(g_mutex);
  pm_handle* h = Context();
  DeviceBuffer d_in(h, Bytes(bgr)), d_r(h, Bytes(range)), d_out(h, Bytes(bgr));
  d_in.Upload(bgr.data(), Bytes(bgr));
  d_r.Upload(range.data(), Bytes(range));
  Check(pm_remove_backscatter(h, d_in.as<float>(), d_r.as<float>(), bgr.rows, bgr.cols, B.data(), beta_B.data(),
                              d_out.as<float>()),
        "pm_remove_backscatter");
  Image3f out(bgr.rows, bgr.cols);
  d_out.Download(out.data(), Bytes(out));
  return out;
}

Image3f CorrectAttenuation(const Image3f& bgr, const Image1f& range, const Vector12f& X) {
  SameSize(bgr.rows, bgr.cols, range.rows, range.cols, "CorrectAttenuation");
  std::lock_guard<std::mutex> lock(g_mutex);
  pm_handle* h = Context();
  DeviceBuffer d_in(h, Bytes(bgr)), d_r(h, Bytes(range)), d_out(h, Bytes(bgr));
  d_in.Upload(bgr.data(), Bytes(bgr));
  d_r.Upload(range.data(), Bytes(range));
  Check(pm_correct_attenuation(h, d_in.as<float>(), d_r.as<float>(), bgr.rows, bgr.cols, X.data(), d_out.as<float>()),
        "pm_correct_attenuation");
  Image3f out(bgr.rows, bgr.cols);
  d_out.Download(out.data(), Bytes(out));
  return out;
}

Image1b StereoReady(const Image3b& bgr) {
  std::lock_guard<std::mutex> lock(g_mutex);
  pm_handle* h = Context();
  DeviceBuffer d_in(h, Bytes(bgr)), d_g(h, (size_t)bgr.rows * bgr.cols);
  d_in.Upload(bgr.data(), Bytes(bgr));
  Check(pm_stereo_ready(h, d_in.as<uint8_t>(), bgr.rows, bgr.cols, nullptr, d_g.as<uint8_t>()), "pm_stereo_ready");
  Image1b out(bgr.rows, bgr.cols);
  d_g.Download(out.data(), Bytes(out));
  return out;
}

Image1f DispToDepth(const Image1f& disp, double fx, double baseline) {
  std::lock_guard<std::mutex> lock(g_mutex);
  pm_handle* h = Context();
  DeviceBuffer d_in(h, Bytes(disp)), d_out(h, Bytes(disp));
  d_in.Upload(disp.data(), Bytes(disp));
  Check(pm_disp_to_range(h, d_in.as<float>(), disp.rows, disp.cols, fx, baseline, d_out.as<float>()),
        "pm_disp_to_range");
  Image1f out(disp.rows, disp.cols);
  d_out.Download(out.data(), Bytes(out));
  return out;
}

double StereoRectify(const CameraModel& cam1, const CameraModel& cam2, const std::array<double, 9>& R,
                     const std::array<double, 3>& T, RectifyView* view1, RectifyView* view2) {
  const pm_camera c1{cam1.fx, cam1.fy, cam1.cx, cam1.cy, cam1.k1, cam1.k2, cam1.p1, cam1.p2, cam1.k3};
  const pm_camera c2{cam2.fx, cam2.fy, cam2.cx, cam2.cy, cam2.k1, cam2.k2, cam2.p1, cam2.p2, cam2.k3};
  double baseline = 0;
  if (pm_stereo_rectify(&c1, &c2, R.data(), T.data(), view1, view2, &baseline) != PM_OK)
    throw std::invalid_argument("StereoRectify: null view, non-finite calibration, or camera 1 is not the left camera");
  return baseline;
}

namespace {

// Both Rectify overloads: Pixel is uint8_t (pm_rectify_u8) or the three interleaved bytes of core::Vec3b (pm_rectify_bgr8).
template <typename Pixel>
Image<Pixel> RectifyImage(const Image<Pixel>& raw, const RectifyView& view, int rows, int cols, Image1b* valid) {
  static_assert(sizeof(Pixel) == 1 || sizeof(Pixel) == 3, "gray, or interleaved BGR bytes");
  if (raw.rows <= 0 || raw.cols <= 0 || rows <= 0 || cols <= 0) throw std::invalid_argument("Rectify: empty image");
  std::lock_guard<std::mutex> lock(g_mutex);
  pm_handle* h = Context();
  Image<Pixel> out(rows, cols);
  const size_t px = (size_t)rows * cols;
  DeviceBuffer d_in(h, Bytes(raw)), d_out(h, Bytes(out)), d_valid(h, px);
  d_in.Upload(raw.data(), Bytes(raw));
  uint8_t* d_mask = valid ? d_valid.as<uint8_t>() : nullptr;
  if constexpr (sizeof(Pixel) == 1)
    Check(pm_rectify_u8(h, &view, d_in.as<uint8_t>(), 1, raw.rows, raw.cols, 0, rows, cols, 0, d_out.as<uint8_t>(), d_mask,
                        nullptr),
          "pm_rectify_u8");
  else
    Check(pm_rectify_bgr8(h, &view, d_in.as<uint8_t>(), 1, raw.rows, raw.cols, 0, rows, cols, 0, d_out.as<uint8_t>(), nullptr,
                          d_mask, nullptr),
          "pm_rectify_bgr8");
  d_out.Download(out.data(), Bytes(out));
  if (valid) d_valid.DownloadInto(valid, rows, cols);
  return out;
}

}  // namespace

Image1b Rectify(const Image1b& raw, const RectifyView& view, int rows, int cols, Image1b* valid) {
  return RectifyImage(raw, view, rows, cols, valid);
}

core::Image<core::Vec3b> Rectify(const core::Image<core::Vec3b>& raw, const RectifyView& view, int rows, int cols,
                                 core::Image<uint8_t>* valid) {
  return RectifyImage(raw, view, rows, cols, valid);
}

namespace {
pm_cloud_camera CloudCamera(const StereoModel& m) { return pm_cloud_camera{m.fx, m.fy, m.cx, m.cy, m.baseline}; }
}  // namespace

core::Image<core::Vec3f> Backproject(const core::Image<float>& disp, const StereoModel& model) {
  if (disp.rows <= 0 || disp.cols <= 0) throw std::invalid_argument("Backproject: empty map");
  std::lock_guard<std::mutex> lock(g_mutex);
  pm_handle* h = Context();
  core::Image<core::Vec3f> out(disp.rows, disp.cols);
  DeviceBuffer d_in(h, Bytes(disp)), d_out(h, Bytes(out));
  d_in.Upload(disp.data(), Bytes(disp));
  const pm_cloud_camera cam = CloudCamera(model);
  Check(pm_backproject(h, &cam, d_in.as<float>(), disp.rows, disp.cols, d_out.as<float>()), "pm_backproject");
  d_out.Download(out.data(), Bytes(out));
  return out;
}

namespace {

// What MakePointCloud and MakeGridMesh share: the size checks (`who` names the caller), ...
void CheckCloudSizes(const std::string& who, const core::Image<float>& disp, const core::Image<core::Vec3f>* normals,
                     const core::Image<core::Vec3b>* bgr) {
  if (disp.rows <= 0 || disp.cols <= 0) throw std::invalid_argument(who + ": empty map");
  if (normals) SameSize(disp.rows, disp.cols, normals->rows, normals->cols, (who + " (normals)").c_str());
  if (bgr) SameSize(disp.rows, disp.cols, bgr->rows, bgr->cols, (who + " (bgr)").c_str());
}

// ... the inputs on the device (normals / bgr null where not given) with the camera and the filter of the C ABI, ...
struct CloudInputs {
  CloudInputs(pm_handle* h, const core::Image<float>& disp_in, const StereoModel& model, const CloudFilter& filter,
              const core::Image<core::Vec3f>* n, const core::Image<core::Vec3b>* c)
      : d_in(h, Bytes(disp_in)), d_n(h, n ? Bytes(*n) : 0), d_c(h, c ? Bytes(*c) : 0), disp(d_in.as<float>()),
        normals(n ? d_n.as<float>() : nullptr), bgr(c ? d_c.as<uint8_t>() : nullptr), cam(CloudCamera(model)),
        flt{filter.min_disp, filter.max_range, filter.stride} {
    d_in.Upload(disp_in.data(), Bytes(disp_in));
    if (n) d_n.Upload(n->data(), Bytes(*n));
    if (c) d_c.Upload(c->data(), Bytes(*c));
  }
  DeviceBuffer d_in, d_n, d_c;
  float* const disp;
  float* const normals;
  uint8_t* const bgr;
  const pm_cloud_camera cam;
  const pm_cloud_filter flt;
};

// ... and the four vertex streams of `n` records, which come back into a PointCloud.
struct VertexStreams {
  VertexStreams(pm_handle* h, size_t n, const CloudInputs& in)
      : n(n), o_xyz(h, n * sizeof(core::Vec3f)), o_n(h, in.normals ? n * sizeof(core::Vec3f) : 0),
        o_c(h, in.bgr ? n * sizeof(core::Vec3b) : 0), o_i(h, n * sizeof(int32_t)), xyz(o_xyz.as<float>()),
        normals(in.normals ? o_n.as<float>() : nullptr), bgr(in.bgr ? o_c.as<uint8_t>() : nullptr), index(o_i.as<int32_t>()) {}
  void Download(PointCloud* pc) {
    pc->xyz.resize(n);
    pc->index.resize(n);
    o_xyz.Download(pc->xyz.data(), n * sizeof(core::Vec3f));
    o_i.Download(pc->index.data(), n * sizeof(int32_t));
    if (normals) {
      pc->normals.resize(n);
      o_n.Download(pc->normals.data(), n * sizeof(core::Vec3f));
    }
    if (bgr) {
      pc->bgr.resize(n);
      o_c.Download(pc->bgr.data(), n * sizeof(core::Vec3b));
    }
  }
  const size_t n;
  DeviceBuffer o_xyz, o_n, o_c, o_i;
  float* const xyz;
  float* const normals;
  uint8_t* const bgr;
  int32_t* const index;
};

}  // namespace

PointCloud MakePointCloud(const core::Image<float>& disp, const StereoModel& model, const CloudFilter& filter,
                          const core::Image<core::Vec3f>* normals, const core::Image<core::Vec3b>* bgr) {
  CheckCloudSizes("MakePointCloud", disp, normals, bgr);
  std::lock_guard<std::mutex> lock(g_mutex);
  pm_handle* h = Context();
  CloudInputs in(h, disp, model, filter, normals, bgr);
  // count first (capacity 0), then outputs of exactly that size
  int count = 0;
  Check(pm_point_cloud(h, &in.cam, &in.flt, in.disp, nullptr, nullptr, disp.rows, disp.cols, 0, nullptr, nullptr, nullptr,
                       nullptr, nullptr, &count),
        "pm_point_cloud");
  PointCloud pc;
  if (count <= 0) return pc;
  VertexStreams out(h, (size_t)count, in);
  int again = 0;
  Check(pm_point_cloud(h, &in.cam, &in.flt, in.disp, in.normals, in.bgr, disp.rows, disp.cols, count, out.xyz, out.normals,
                       out.bgr, out.index, nullptr, &again),
        "pm_point_cloud");
  if (again != count) throw std::runtime_error("MakePointCloud: the count changed between two passes over one map");
  out.Download(&pc);
  return pc;
}

TriangleMesh MakeGridMesh(const core::Image<float>& disp, const StereoModel& model, const CloudFilter& filter,
                          const MeshOptions& options, const core::Image<core::Vec3f>* normals,
                          const core::Image<core::Vec3b>* bgr) {
  CheckCloudSizes("MakeGridMesh", disp, normals, bgr);
  std::lock_guard<std::mutex> lock(g_mutex);
  pm_handle* h = Context();
  CloudInputs in(h, disp, model, filter, normals, bgr);
  const pm_mesh_options opt = {options.max_diff, options.referenced_vertices ? PM_MESH_VERTICES_REFERENCED : PM_MESH_VERTICES_ALL};
  // count first (both capacities 0), then outputs of exactly that size
  int counts[2] = {0, 0};
  Check(pm_grid_mesh(h, &in.cam, &in.flt, &opt, in.disp, nullptr, nullptr, disp.rows, disp.cols, 0, 0, nullptr, nullptr,
                     nullptr, nullptr, nullptr, nullptr, counts),
        "pm_grid_mesh");
  TriangleMesh mesh;
  if (counts[0] <= 0) return mesh;
  const size_t t = (size_t)(counts[1] > 0 ? counts[1] : 0);
  VertexStreams out(h, (size_t)counts[0], in);
  DeviceBuffer o_t(h, t * 3 * sizeof(int32_t));
  int again[2] = {0, 0};
  Check(pm_grid_mesh(h, &in.cam, &in.flt, &opt, in.disp, in.normals, in.bgr, disp.rows, disp.cols, counts[0], counts[1],
                     out.xyz, out.normals, out.bgr, out.index, t ? o_t.as<int32_t>() : nullptr, nullptr, again),
        "pm_grid_mesh");
  if (again[0] != counts[0] || again[1] != counts[1])
    throw std::runtime_error("MakeGridMesh: the counts changed between two passes over one map");
  out.Download(&mesh.vertices);
  mesh.triangles.resize(t);
  if (t) o_t.Download(mesh.triangles.data(), t * 3 * sizeof(int32_t));
  return mesh;
}

void WritePly(const std::string& path, const TriangleMesh& mesh) {
  const PointCloud& pc = mesh.vertices;
  const size_t n = pc.xyz.size();
  const bool has_n = !pc.normals.empty(), has_c = !pc.bgr.empty();
  if ((has_n && pc.normals.size() != n) || (has_c && pc.bgr.size() != n))
    throw std::invalid_argument("WritePly: the vertex streams differ in length");
  std::string head = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(n) +
                     "\nproperty float x\nproperty float y\nproperty float z\n";
  if (has_n) head += "property float nx\nproperty float ny\nproperty float nz\n";
  if (has_c) head += "property uchar red\nproperty uchar green\nproperty uchar blue\n";
  head += "element face " + std::to_string(mesh.triangles.size()) + "\nproperty list uchar int vertex_indices\nend_header\n";
  // the records are assembled byte by byte (binary32 and int32 are little-endian on every host this library builds for)
  const size_t vbytes = 12 + (has_n ? 12 : 0) + (has_c ? 3 : 0);
  std::vector<uint8_t> body(n * vbytes + mesh.triangles.size() * 13);
  uint8_t* o = body.data();
  for (size_t i = 0; i < n; ++i) {
    std::memcpy(o, &pc.xyz[i], 12), o += 12;
    if (has_n) std::memcpy(o, &pc.normals[i], 12), o += 12;
    if (has_c) *o++ = pc.bgr[i].v[2], *o++ = pc.bgr[i].v[1], *o++ = pc.bgr[i].v[0];  // B G R -> red green blue
  }
  for (const std::array<int32_t, 3>& t : mesh.triangles) {
    *o++ = 3;
    std::memcpy(o, t.data(), 12), o += 12;
  }
  FILE* f = std::fopen(path.c_str(), "wb");
  bool ok = f != nullptr;
  ok = ok && std::fwrite(head.data(), 1, head.size(), f) == head.size();
  ok = ok && (body.empty() || std::fwrite(body.data(), 1, body.size(), f) == body.size());
  if (f) ok = (std::fclose(f) == 0) && ok;
  if (!ok) throw std::runtime_error("WritePly: cannot write " + path);
}

Motion RelativeMotion(const double T_world_old[16], const double T_world_new[16]) {
  // with T = [R | p]:  T_new^-1 = [Rn^T | -Rn^T pn], so  R = Rn^T Ro  and  t = Rn^T (po - pn)
  const double* A = T_world_old;
  const double* B = T_world_new;
  Motion m;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      double s = 0;
      for (int k = 0; k < 3; ++k) s += B[4 * k + i] * A[4 * k + j];
      m.R[(size_t)(3 * i + j)] = s;
    }
    double s = 0;
    for (int k = 0; k < 3; ++k) s += B[4 * k + i] * (A[4 * k + 3] - B[4 * k + 3]);
    m.t[(size_t)i] = s;
  }
  return m;
}

std::array<int, 2> ReprojectDisparity(pm::PatchmatchGpu& matcher, const StereoModel& model, const Motion& motion,
                                      const float* d_disp, int rows, int cols, float* d_seed_l, float* d_seed_r,
                                      const ReprojectOptions& options, bool want_counts) {
  pm_handle* h = MatcherHandle(matcher, "ReprojectDisparity");
  const pm_cloud_camera cam = CloudCamera(model);
  const pm_motion m = ToC(motion);
  const pm_reproject_options opt = {options.min_disp, options.max_disp, options.close_radius};
  int counts[2] = {-1, -1};
  CheckOn(h, pm_reproject_disparity(h, &cam, &m, &opt, d_disp, rows, cols, d_seed_l, d_seed_r, nullptr, want_counts ? counts : nullptr),
          "pm_reproject_disparity");
  return {{counts[0], counts[1]}};
}

std::array<int, 2> FilterConsistency(pm::PatchmatchGpu& matcher, const StereoModel& model,
                                     const std::vector<core::Image<float>>& sources, const std::vector<Motion>& motions,
                                     const ConsistencyOptions& options, const core::Image<float>& disp,
                                     core::Image<float>* out, core::Image<uint16_t>* classes, core::Image<float>* residual) {
  DeviceBuffers dev(MatcherHandle(matcher, "FilterConsistency"));
  const int rows = disp.rows, cols = disp.cols;
  if (rows <= 0 || cols <= 0) throw std::invalid_argument("FilterConsistency: empty map");
  if (sources.size() != motions.size()) throw std::invalid_argument("FilterConsistency: one motion per source");
  for (const core::Image<float>& s : sources) SameSize(rows, cols, s.rows, s.cols, "FilterConsistency");
  const size_t px = (size_t)rows * cols;
  float* d_disp = dev.Put<float>(disp.data(), 4 * px);
  std::vector<const float*> d_sources;
  std::vector<pm_motion> m;
  for (size_t k = 0; k < sources.size(); ++k) {
    d_sources.push_back(dev.Put<float>(sources[k].data(), 4 * px));
    m.push_back(ToC(motions[k]));
  }
  uint16_t* d_classes = classes ? dev.Get<uint16_t>(2 * px) : nullptr;
  float* d_residual = residual ? dev.Get<float>(4 * px) : nullptr;
  const pm_cloud_camera cam = CloudCamera(model);
  const pm_consistency_options opt = {options.max_diff, options.radius, options.min_consistent, options.max_conflicts};
  int counts[2] = {-1, -1};
  dev.Check(pm_filter_consistency(dev.handle(), &cam, &opt, d_disp, (int)sources.size(), d_sources.data(), m.data(), rows, cols,
                                  out ? d_disp : nullptr /* in place on the device */, d_classes, d_residual, nullptr, counts),
            "pm_filter_consistency");
  if (out) dev.Fetch(out, d_disp, rows, cols);
  if (classes) dev.Fetch(classes, d_classes, rows, cols);
  if (residual) dev.Fetch(residual, d_residual, rows, cols);
  return {{counts[0], counts[1]}};
}

std::array<int, 3> DisparityConfidence(pm::PatchmatchGpu& matcher, const core::Image<uint8_t>& left,
                                       const core::Image<uint8_t>& right, const ConfidenceOptions& options,
                                       const core::Image<float>& disp_l, const core::Image<float>* disp_r,
                                       core::Image<float>* out, ConfidenceMeasures* measures, core::Image<uint8_t>* flags) {
  DeviceBuffers dev(MatcherHandle(matcher, "DisparityConfidence"));
  const int rows = disp_l.rows, cols = disp_l.cols;
  if (rows <= 0 || cols <= 0) throw std::invalid_argument("DisparityConfidence: empty map");
  SameSize(rows, cols, left.rows, left.cols, "DisparityConfidence");
  SameSize(rows, cols, right.rows, right.cols, "DisparityConfidence");
  if (disp_r) SameSize(rows, cols, disp_r->rows, disp_r->cols, "DisparityConfidence");
  if (left.step != (size_t)cols || right.step != (size_t)cols) throw std::invalid_argument("DisparityConfidence: the images must be packed");
  const size_t px = (size_t)rows * cols;
  const uint8_t* d_left = dev.Put<uint8_t>(left.data(), px);
  const uint8_t* d_right = dev.Put<uint8_t>(right.data(), px);
  float* d_disp = dev.Put<float>(disp_l.data(), 4 * px);
  const float* d_disp_r = disp_r ? dev.Put<float>(disp_r->data(), 4 * px) : nullptr;
  float* d_measures = measures ? dev.Get<float>(16 * px) : nullptr;
  uint8_t* d_flags = flags ? dev.Get<uint8_t>(px) : nullptr;
  const pm_confidence_options opt = {options.patch_w,    options.patch_h,     options.max_cost,           options.min_margin,
                                     options.min_bg_margin, options.max_lr_diff, options.drop_unmeasured ? 1 : 0};
  int counts[3] = {-1, -1, -1};
  dev.Check(pm_disparity_confidence(dev.handle(), &opt, d_left, d_right, d_disp, d_disp_r, rows, cols,
                                    out ? d_disp : nullptr /* in place on the device */, d_measures, d_flags, nullptr, counts),
            "pm_disparity_confidence");
  if (out) dev.Fetch(out, d_disp, rows, cols);
  if (measures) {
    dev.Fetch(&measures->cost, d_measures, rows, cols);
    dev.Fetch(&measures->margin, d_measures + px, rows, cols);
    dev.Fetch(&measures->bg_margin, d_measures + 2 * px, rows, cols);
    dev.Fetch(&measures->lr, d_measures + 3 * px, rows, cols);
  }
  if (flags) dev.Fetch(flags, d_flags, rows, cols);
  return {{counts[0], counts[1], counts[2]}};
}

std::array<int, 4> FuseDisparity(pm::PatchmatchGpu& matcher, const StereoModel& model,
                                 const std::vector<core::Image<float>>& sources, const std::vector<Motion>& motions,
                                 const FuseOptions& options, const core::Image<float>& disp, const core::Image<float>* weight,
                                 const std::vector<core::Image<float>>& source_weights, core::Image<float>* out,
                                 core::Image<uint8_t>* count, core::Image<float>* spread, core::Image<uint8_t>* flags) {
  DeviceBuffers dev(MatcherHandle(matcher, "FuseDisparity"));
  const int rows = disp.rows, cols = disp.cols;
  if (rows <= 0 || cols <= 0) throw std::invalid_argument("FuseDisparity: empty map");
  if (sources.size() != motions.size()) throw std::invalid_argument("FuseDisparity: one motion per source");
  if (!source_weights.empty() && source_weights.size() != sources.size())
    throw std::invalid_argument("FuseDisparity: source_weights is empty or has one entry per source");
  for (const core::Image<float>& s : sources) SameSize(rows, cols, s.rows, s.cols, "FuseDisparity");
  if (weight) SameSize(rows, cols, weight->rows, weight->cols, "FuseDisparity");
  for (const core::Image<float>& w : source_weights)
    if (w.rows != 0 || w.cols != 0) SameSize(rows, cols, w.rows, w.cols, "FuseDisparity");
  const size_t px = (size_t)rows * cols;
  float* d_disp = dev.Put<float>(disp.data(), 4 * px);
  const float* d_weight = weight ? dev.Put<float>(weight->data(), 4 * px) : nullptr;
  std::vector<const float*> d_sources, d_weights;
  std::vector<pm_motion> m;
  for (size_t k = 0; k < sources.size(); ++k) {
    d_sources.push_back(dev.Put<float>(sources[k].data(), 4 * px));
    const bool has = !source_weights.empty() && source_weights[k].rows != 0;
    d_weights.push_back(has ? dev.Put<float>(source_weights[k].data(), 4 * px) : nullptr);
    m.push_back(ToC(motions[k]));
  }
  uint8_t* d_count = count ? dev.Get<uint8_t>(px) : nullptr;
  float* d_spread = spread ? dev.Get<float>(4 * px) : nullptr;
  uint8_t* d_flags = flags ? dev.Get<uint8_t>(px) : nullptr;
  const pm_cloud_camera cam = CloudCamera(model);
  const pm_fuse_options opt = {options.max_diff,      options.radius,           options.min_consistent,
                               options.max_conflicts, options.fill_min_sources, options.fill_max_diff};
  int counts[4] = {-1, -1, -1, -1};
  dev.Check(pm_fuse_disparity(dev.handle(), &cam, &opt, d_disp, d_weight, (int)sources.size(), d_sources.data(), m.data(),
                              source_weights.empty() ? nullptr : d_weights.data(), rows, cols,
                              out ? d_disp : nullptr /* in place on the device */, d_count, d_spread, d_flags, nullptr, counts),
            "pm_fuse_disparity");
  if (out) dev.Fetch(out, d_disp, rows, cols);
  if (count) dev.Fetch(count, d_count, rows, cols);
  if (spread) dev.Fetch(spread, d_spread, rows, cols);
  if (flags) dev.Fetch(flags, d_flags, rows, cols);
  return {{counts[0], counts[1], counts[2], counts[3]}};
}

namespace {
// The two frames of a motion estimate on the matcher's handle (not the imaging context's); every buffer is freed on every way
// out.
struct MotionFrames {
  DeviceBuffers dev;
  pm_handle* const h;
  const uint8_t *old = nullptr, *img = nullptr;
  const float* disp = nullptr;
  const pm_cloud_camera cam;
  const pm_track_options opt;
  const pm_motion guess;
  MotionFrames(pm::PatchmatchGpu& matcher, const char* who, const StereoModel& model, const TrackOptions& o, const Motion* g,
               const core::Image<uint8_t>& left_old, const core::Image<float>& disp_old, const core::Image<uint8_t>& left_new)
      : dev(MatcherHandle(matcher, who)), h(dev.handle()), cam(CloudCamera(model)),
        opt{o.cell, o.patch_radius, o.search_radius, o.min_score, o.min_disp, o.max_disp, o.max_sad, o.min_gap},
        guess(ToC(g ? *g : Motion())) {
    SameSize(left_old.rows, left_old.cols, disp_old.rows, disp_old.cols, who);
    SameSize(left_old.rows, left_old.cols, left_new.rows, left_new.cols, who);
    old = dev.Put<uint8_t>(left_old.data(), Bytes(left_old));
    disp = dev.Put<float>(disp_old.data(), Bytes(disp_old));
    img = dev.Put<uint8_t>(left_new.data(), Bytes(left_new));
  }
};
}  // namespace

std::vector<pm_track> TrackFeatures(pm::PatchmatchGpu& matcher, const StereoModel& model, const TrackOptions& options,
                                    const Motion* guess, const core::Image<uint8_t>& left_old, const core::Image<float>& disp_old,
                                    const core::Image<uint8_t>& left_new) {
  MotionFrames f(matcher, "TrackFeatures", model, options, guess, left_old, disp_old, left_new);
  const int rows = left_old.rows, cols = left_old.cols;
  // at most one feature per cell: room for all of them without a counting call in front
  const int cell = options.cell > 0 ? options.cell : 1;
  const int capacity = ((rows + cell - 1) / cell) * ((cols + cell - 1) / cell);
  pm_track* d_tracks = f.dev.Get<pm_track>(sizeof(pm_track) * (size_t)capacity);
  int count = -1;
  f.dev.Check(pm_track_features(f.h, &f.cam, &f.opt, &f.guess, f.old, f.disp, f.img, rows, cols, capacity, d_tracks, nullptr, &count),
              "pm_track_features");
  std::vector<pm_track> tracks((size_t)count);
  if (count > 0) f.dev.Check(pm_download(f.h, tracks.data(), d_tracks, sizeof(pm_track) * tracks.size()), "pm_download");
  return tracks;
}

Motion SolveMotion(const StereoModel& model, const SolveOptions& options, const std::vector<pm_track>& tracks, const Motion* guess,
                   pm_motion_info* info) {
  const pm_cloud_camera cam = CloudCamera(model);
  const pm_solve_options opt = {options.iterations, options.huber_px, options.epsilon, options.inlier_px, options.min_inliers};
  const pm_motion g = ToC(guess ? *guess : Motion());
  pm_motion out;
  pm_motion_info local;
  const int rc = pm_solve_motion(&cam, &opt, tracks.data(), (int)tracks.size(), &g, &out, info ? info : &local);
  if (rc != PM_OK) throw std::runtime_error(std::string("pm_solve_motion: ") + pm_status_string(rc));
  return FromC(out);
}

Motion EstimateMotion(pm::PatchmatchGpu& matcher, const StereoModel& model, const TrackOptions& track_options,
                      const SolveOptions& solve_options, const Motion* guess, const core::Image<uint8_t>& left_old,
                      const core::Image<float>& disp_old, const core::Image<uint8_t>& left_new, pm_motion_info* info) {
  MotionFrames f(matcher, "EstimateMotion", model, track_options, guess, left_old, disp_old, left_new);
  const pm_solve_options opt = {solve_options.iterations, solve_options.huber_px, solve_options.epsilon, solve_options.inlier_px,
                                solve_options.min_inliers};
  pm_motion out;
  pm_motion_info local;
  f.dev.Check(pm_estimate_motion(f.h, &f.cam, &f.opt, &opt, &f.guess, f.old, f.disp, f.img, left_old.rows, left_old.cols, &out,
                                 info ? info : &local),
              "pm_estimate_motion");
  return FromC(out);
}

namespace {
pm_align_options ToC(const AlignOptions& o) {
  return pm_align_options{o.min_disp, o.max_diff, o.huber_px, o.iterations, o.epsilon, o.min_used};
}
}  // namespace

Motion AlignDisparity(pm::PatchmatchGpu& matcher, const StereoModel& model, const AlignOptions& options, const Motion* guess,
                      const core::Image<float>& disp_model, const core::Image<core::Vec3f>& normals_model,
                      const core::Image<float>& disp_new, pm_align_info* info) {
  const char* const who = "AlignDisparity";
  DeviceBuffers dev(MatcherHandle(matcher, who));
  if (disp_model.rows <= 0 || disp_model.cols <= 0) throw std::invalid_argument("AlignDisparity: empty map");
  SameSize(disp_model.rows, disp_model.cols, normals_model.rows, normals_model.cols, who);
  SameSize(disp_model.rows, disp_model.cols, disp_new.rows, disp_new.cols, who);
  const float* d_model = dev.Put<float>(disp_model.data(), Bytes(disp_model));
  const float* d_normals = dev.Put<float>(reinterpret_cast<const float*>(normals_model.data()), Bytes(normals_model));
  const float* d_new = dev.Put<float>(disp_new.data(), Bytes(disp_new));
  const pm_cloud_camera cam = CloudCamera(model);
  const pm_align_options opt = ToC(options);
  const pm_motion g = ToC(guess ? *guess : Motion());
  pm_motion out;
  pm_align_info local;
  dev.Check(pm_align_disparity(dev.handle(), &cam, &opt, &g, d_model, d_normals, d_new, disp_model.rows, disp_model.cols, &out,
                               info ? info : &local),
            "pm_align_disparity");
  return FromC(out);
}

namespace {
pm_align_color_options ToC(const AlignColorOptions& o) { return pm_align_color_options{ToC(o.align), o.huber_levels, o.lambda}; }

// the new image on the device as the one of pm_align_color_disparity's two arguments that its pixel type names
struct NewImage {
  const uint8_t* bgr8 = nullptr;
  const float* bgr = nullptr;
  NewImage(DeviceBuffers& dev, const core::Image<core::Vec3b>& image)
      : bgr8(dev.Put<uint8_t>(reinterpret_cast<const uint8_t*>(image.data()), Bytes(image))) {}
  NewImage(DeviceBuffers& dev, const core::Image<core::Vec3f>& image)
      : bgr(dev.Put<float>(reinterpret_cast<const float*>(image.data()), Bytes(image))) {}
};

template <typename Pixel>
Motion AlignColorHost(pm::PatchmatchGpu& matcher, const StereoModel& model, const AlignColorOptions& options, const Motion* guess,
                      const core::Image<float>& disp_model, const core::Image<core::Vec3f>& normals_model,
                      const core::Image<core::Vec3f>& bgr_model, const core::Image<float>& disp_new,
                      const core::Image<Pixel>& bgr_new, pm_align_color_info* info) {
  const char* const who = "AlignColorDisparity";
  DeviceBuffers dev(MatcherHandle(matcher, who));
  const int rows = disp_model.rows, cols = disp_model.cols;
  if (rows <= 0 || cols <= 0) throw std::invalid_argument("AlignColorDisparity: empty map");
  SameSize(rows, cols, normals_model.rows, normals_model.cols, who);
  SameSize(rows, cols, bgr_model.rows, bgr_model.cols, who);
  SameSize(rows, cols, disp_new.rows, disp_new.cols, who);
  SameSize(rows, cols, bgr_new.rows, bgr_new.cols, who);
  const float* d_model = dev.Put<float>(disp_model.data(), Bytes(disp_model));
  const float* d_normals = dev.Put<float>(reinterpret_cast<const float*>(normals_model.data()), Bytes(normals_model));
  const float* d_bgr_model = dev.Put<float>(reinterpret_cast<const float*>(bgr_model.data()), Bytes(bgr_model));
  const float* d_new = dev.Put<float>(disp_new.data(), Bytes(disp_new));
  const NewImage image(dev, bgr_new);
  const pm_cloud_camera cam = CloudCamera(model);
  const pm_align_color_options opt = ToC(options);
  const pm_motion g = ToC(guess ? *guess : Motion());
  pm_motion out;
  pm_align_color_info local;
  dev.Check(pm_align_color_disparity(dev.handle(), &cam, &opt, &g, d_model, d_normals, d_bgr_model, d_new, image.bgr8, image.bgr, rows,
                                     cols, &out, info ? info : &local),
            "pm_align_color_disparity");
  return FromC(out);
}
}  // namespace

Motion AlignColorDisparity(pm::PatchmatchGpu& matcher, const StereoModel& model, const AlignColorOptions& options,
                           const Motion* guess, const core::Image<float>& disp_model, const core::Image<core::Vec3f>& normals_model,
                           const core::Image<core::Vec3f>& bgr_model, const core::Image<float>& disp_new,
                           const core::Image<core::Vec3b>& bgr_new, pm_align_color_info* info) {
  return AlignColorHost(matcher, model, options, guess, disp_model, normals_model, bgr_model, disp_new, bgr_new, info);
}

Motion AlignColorDisparity(pm::PatchmatchGpu& matcher, const StereoModel& model, const AlignColorOptions& options,
                           const Motion* guess, const core::Image<float>& disp_model, const core::Image<core::Vec3f>& normals_model,
                           const core::Image<core::Vec3f>& bgr_model, const core::Image<float>& disp_new,
                           const core::Image<core::Vec3f>& bgr_new, pm_align_color_info* info) {
  return AlignColorHost(matcher, model, options, guess, disp_model, normals_model, bgr_model, disp_new, bgr_new, info);
}

Motion ComposeMotion(const Motion& a, const Motion& b) {
  const pm_motion ca = ToC(a), cb = ToC(b);
  pm_motion out;
  const int rc = pm_motion_compose(&ca, &cb, &out);
  if (rc != PM_OK) throw std::runtime_error(std::string("pm_motion_compose: ") + pm_status_string(rc));
  return FromC(out);
}

core::Image<core::Vec3f> DisparityNormals(const core::Image<float>& disp, const StereoModel& model, const NormalsFit& fit,
                                          core::Image<uint8_t>* support) {
  if (disp.rows <= 0 || disp.cols <= 0) throw std::invalid_argument("DisparityNormals: empty map");
  std::lock_guard<std::mutex> lock(g_mutex);
  pm_handle* h = Context();
  core::Image<core::Vec3f> out(disp.rows, disp.cols);
  const size_t px = (size_t)disp.rows * disp.cols;
  DeviceBuffer d_in(h, Bytes(disp)), d_out(h, Bytes(out)), d_sup(h, support ? px : 0);
  d_in.Upload(disp.data(), Bytes(disp));
  const pm_cloud_camera cam = CloudCamera(model);
  const pm_normals_fit f = {fit.radius, fit.max_diff, fit.min_support};
  Check(pm_disparity_normals(h, &cam, &f, d_in.as<float>(), disp.rows, disp.cols, d_out.as<float>(), nullptr,
                             support ? d_sup.as<uint8_t>() : nullptr),
        "pm_disparity_normals");
  d_out.Download(out.data(), Bytes(out));
  if (support) d_sup.DownloadInto(support, disp.rows, disp.cols);
  return out;
}

core::Image<float> FilterSpeckles(const core::Image<float>& disp, const SpeckleFilter& filter, core::Image<int32_t>* labels,
                                  int* removed) {
  if (disp.rows <= 0 || disp.cols <= 0) throw std::invalid_argument("FilterSpeckles: empty map");
  std::lock_guard<std::mutex> lock(g_mutex);
  pm_handle* h = Context();
  core::Image<float> out(disp.rows, disp.cols);
  const size_t px = (size_t)disp.rows * disp.cols;
  DeviceBuffer d_map(h, Bytes(disp)), d_lab(h, labels ? sizeof(int32_t) * px : 0);
  d_map.Upload(disp.data(), Bytes(disp));
  const pm_speckle_filter f = {filter.max_diff, filter.max_size};
  Check(pm_filter_speckles(h, &f, d_map.as<float>(), disp.rows, disp.cols, d_map.as<float>(),  // in place on the device
                           labels ? d_lab.as<int32_t>() : nullptr, nullptr, nullptr, removed),
        "pm_filter_speckles");
  d_map.Download(out.data(), Bytes(out));
  if (labels) d_lab.DownloadInto(labels, disp.rows, disp.cols);
  return out;
}

core::Image<core::Vec3f> PlaneNormals(pm::PatchmatchGpu& matcher, const StereoModel& model, int rows, int cols,
                                      const core::Image<float>* disp_l) {
  pm_handle* h = matcher.handle();
  if (!h) throw std::runtime_error("PlaneNormals: the matcher has not matched yet");
  if (rows <= 0 || cols <= 0) throw std::invalid_argument("PlaneNormals: empty size");
  if (disp_l) SameSize(rows, cols, disp_l->rows, disp_l->cols, "PlaneNormals");
  DeviceBuffers dev(h);  // the matcher's handle, not the imaging context's
  core::Image<core::Vec3f> out(rows, cols);
  float* d_out = dev.Get<float>(Bytes(out));
  const float* d_mask = disp_l ? dev.Put<float>(disp_l->data(), Bytes(*disp_l)) : nullptr;
  const pm_cloud_camera cam = CloudCamera(model);
  dev.Check(pm_planes_normals(h, 0, &cam, d_mask, rows, cols, d_out), "pm_planes_normals");
  dev.Fetch(&out, d_out, rows, cols);
  return out;
}

// ---- TsdfVolume: the device memory is on the matcher's handle, and so is every call -------------------------------------------
struct TsdfVolume::Impl {
  DeviceBuffers dev;
  pm_handle* const h;
  const pm_tsdf_volume volume;
  void* const voxels;
  void* const colors;  // null without a colour volume
  // Align's render and the new map on the device, kept from call to call and replaced when a larger map arrives
  float *align_disp = nullptr, *align_normals = nullptr, *align_new = nullptr;
  size_t align_px = 0;
  Impl(pm_handle* handle, const pm_tsdf_volume& v, size_t bytes, size_t color_bytes)
      : dev(handle), h(handle), volume(v), voxels(dev.Get(bytes)), colors(color_bytes ? dev.Get(color_bytes) : nullptr) {}
};

TsdfVolume::TsdfVolume(pm::PatchmatchGpu& matcher, const TsdfGrid& grid, bool with_color) : grid_(grid) {
  pm_handle* h = MatcherHandle(matcher, "TsdfVolume");
  const pm_tsdf_volume v = {grid.nx, grid.ny, grid.nz, {grid.origin[0], grid.origin[1], grid.origin[2]}, grid.voxel, grid.trunc,
                            grid.max_weight};
  const size_t bytes = pm_tsdf_bytes(&v);
  if (bytes == 0) throw std::invalid_argument("TsdfVolume: the grid is invalid or exceeds 2^31 - 1 voxels");
  impl_.reset(new Impl(h, v, bytes, with_color ? pm_tsdf_color_bytes(&v) : 0));
  Clear();
}

TsdfVolume::~TsdfVolume() = default;

void* TsdfVolume::device() { return impl_->voxels; }

bool TsdfVolume::has_color() const { return impl_->colors != nullptr; }

void* TsdfVolume::color_device() { return impl_->colors; }

void TsdfVolume::Clear() {
  impl_->dev.Check(pm_tsdf_clear(impl_->h, &impl_->volume, device()), "pm_tsdf_clear");
  if (has_color()) impl_->dev.Check(pm_tsdf_color_clear(impl_->h, &impl_->volume, color_device()), "pm_tsdf_color_clear");
}

namespace {
void NeedColor(const TsdfVolume& v, const char* who) {
  if (!v.has_color()) throw std::logic_error(std::string(who) + ": the volume was made without a colour volume");
}
}  // namespace

std::array<int, 3> TsdfVolume::IntegrateColorDevice(const StereoModel& model, const Motion& pose, const float* d_disp,
                                                    const float* d_weight, const uint8_t* d_bgr8, const float* d_bgr, int rows,
                                                    int cols, const TsdfColorOptions& options, bool want_counts) {
  NeedColor(*this, "TsdfVolume::IntegrateColor");
  const pm_cloud_camera cam = CloudCamera(model);
  const pm_motion m = ToC(pose);
  const pm_tsdf_color_options opt = {options.min_disp, options.max_range, options.band};
  int counts[3] = {-1, -1, -1};
  impl_->dev.Check(pm_tsdf_integrate_color(impl_->h, &cam, &impl_->volume, &m, &opt, d_disp, d_weight, d_bgr8, d_bgr, rows, cols,
                                           device(), color_device(), nullptr, want_counts ? counts : nullptr),
                   "pm_tsdf_integrate_color");
  return {{counts[0], counts[1], counts[2]}};
}

namespace {
// the host form of IntegrateColor for either pixel type: Pixel is Vec3b (d_bgr8) or Vec3f (d_bgr)
template <typename Pixel>
std::array<int, 3> IntegrateColorHost(TsdfVolume& volume, pm_handle* h, const StereoModel& model, const Motion& pose,
                                      const core::Image<float>& disp, const core::Image<Pixel>& bgr,
                                      const core::Image<float>* weight, const TsdfColorOptions& options) {
  if (disp.rows <= 0 || disp.cols <= 0) throw std::invalid_argument("TsdfVolume::IntegrateColor: empty map");
  SameSize(disp.rows, disp.cols, bgr.rows, bgr.cols, "TsdfVolume::IntegrateColor");
  if (weight) SameSize(disp.rows, disp.cols, weight->rows, weight->cols, "TsdfVolume::IntegrateColor");
  DeviceBuffers dev(h);
  const float* d_disp = dev.Put<float>(disp.data(), Bytes(disp));
  const float* d_weight = weight ? dev.Put<float>(weight->data(), Bytes(*weight)) : nullptr;
  const void* d_image = dev.Put<void>(bgr.data(), Bytes(bgr));
  const bool bytes = sizeof(Pixel) == sizeof(core::Vec3b);
  return volume.IntegrateColorDevice(model, pose, d_disp, d_weight, bytes ? static_cast<const uint8_t*>(d_image) : nullptr,
                                     bytes ? nullptr : static_cast<const float*>(d_image), disp.rows, disp.cols, options,
                                     /*want_counts=*/true);  // synchronises: the buffers may go
}
}  // namespace

std::array<int, 3> TsdfVolume::IntegrateColor(const StereoModel& model, const Motion& pose, const core::Image<float>& disp,
                                              const core::Image<core::Vec3b>& bgr, const core::Image<float>* weight,
                                              const TsdfColorOptions& options) {
  return IntegrateColorHost(*this, impl_->h, model, pose, disp, bgr, weight, options);
}

std::array<int, 3> TsdfVolume::IntegrateColor(const StereoModel& model, const Motion& pose, const core::Image<float>& disp,
                                              const core::Image<core::Vec3f>& bgr, const core::Image<float>* weight,
                                              const TsdfColorOptions& options) {
  return IntegrateColorHost(*this, impl_->h, model, pose, disp, bgr, weight, options);
}

int TsdfVolume::ColorMapDevice(const StereoModel& model, const Motion& pose, const float* d_disp, int rows, int cols,
                               float* d_bgr_out, uint8_t* d_bgr8_out, const TsdfColorSampleOptions& options, bool want_counts) {
  NeedColor(*this, "TsdfVolume::ColorMap");
  const pm_cloud_camera cam = CloudCamera(model);
  const pm_motion m = ToC(pose);
  const pm_tsdf_color_sample_options opt = {options.min_weight, options.byte_scale};
  int colored = -1;
  impl_->dev.Check(pm_tsdf_color_map(impl_->h, &cam, &impl_->volume, &m, &opt, color_device(), d_disp, rows, cols, d_bgr_out,
                                     d_bgr8_out, nullptr, want_counts ? &colored : nullptr),
                   "pm_tsdf_color_map");
  return colored;
}

int TsdfVolume::ColorMap(const StereoModel& model, const Motion& pose, const core::Image<float>& disp,
                         core::Image<core::Vec3f>* bgr, core::Image<core::Vec3b>* bgr8, const TsdfColorSampleOptions& options) {
  if (disp.rows <= 0 || disp.cols <= 0) throw std::invalid_argument("TsdfVolume::ColorMap: empty map");
  if (!bgr && !bgr8) throw std::invalid_argument("TsdfVolume::ColorMap: no output");
  const size_t px = (size_t)disp.rows * disp.cols;
  DeviceBuffers dev(impl_->h);
  const float* d_disp = dev.Put<float>(disp.data(), Bytes(disp));
  float* d_bgr = bgr ? dev.Get<float>(px * sizeof(core::Vec3f)) : nullptr;
  uint8_t* d_bgr8 = bgr8 ? dev.Get<uint8_t>(px * sizeof(core::Vec3b)) : nullptr;
  const int colored = ColorMapDevice(model, pose, d_disp, disp.rows, disp.cols, d_bgr, d_bgr8, options, /*want_counts=*/true);
  if (bgr) dev.Fetch(bgr, d_bgr, disp.rows, disp.cols);
  if (bgr8) dev.Fetch(bgr8, d_bgr8, disp.rows, disp.cols);
  return colored;
}

int TsdfVolume::ColorPoints(const std::vector<core::Vec3f>& xyz, std::vector<core::Vec3f>* bgr, std::vector<core::Vec3b>* bgr8,
                            const TsdfColorSampleOptions& options) {
  NeedColor(*this, "TsdfVolume::ColorPoints");
  if (!bgr && !bgr8) throw std::invalid_argument("TsdfVolume::ColorPoints: no output");
  if (xyz.size() > (size_t)INT32_MAX) throw std::invalid_argument("TsdfVolume::ColorPoints: too many points");
  const size_t n = xyz.size();
  if (bgr) bgr->assign(n, core::Vec3f{{0.f, 0.f, 0.f}});
  if (bgr8) bgr8->assign(n, core::Vec3b{{0, 0, 0}});
  if (n == 0) return 0;
  DeviceBuffers dev(impl_->h);
  const float* d_xyz = dev.Put<float>(xyz.data(), n * sizeof(core::Vec3f));
  float* d_bgr = bgr ? dev.Get<float>(n * sizeof(core::Vec3f)) : nullptr;
  uint8_t* d_bgr8 = bgr8 ? dev.Get<uint8_t>(n * sizeof(core::Vec3b)) : nullptr;
  const pm_tsdf_color_sample_options opt = {options.min_weight, options.byte_scale};
  int colored = -1;
  dev.Check(pm_tsdf_color_points(impl_->h, &impl_->volume, &opt, color_device(), d_xyz, (int)n, nullptr, d_bgr, d_bgr8, nullptr,
                                 &colored),
            "pm_tsdf_color_points");
  if (bgr) dev.Check(pm_download(impl_->h, bgr->data(), d_bgr, n * sizeof(core::Vec3f)), "pm_download");
  if (bgr8) dev.Check(pm_download(impl_->h, bgr8->data(), d_bgr8, n * sizeof(core::Vec3b)), "pm_download");
  return colored;
}

std::array<int, 2> TsdfVolume::IntegrateDevice(const StereoModel& model, const Motion& pose, const float* d_disp,
                                               const float* d_weight, int rows, int cols, const TsdfIntegrateOptions& options,
                                               bool want_counts) {
  const pm_cloud_camera cam = CloudCamera(model);
  const pm_motion m = ToC(pose);
  const pm_tsdf_integrate_options opt = {options.min_disp, options.max_range};
  int counts[2] = {-1, -1};
  impl_->dev.Check(pm_tsdf_integrate(impl_->h, &cam, &impl_->volume, &m, &opt, d_disp, d_weight, rows, cols, device(), nullptr,
                                     want_counts ? counts : nullptr),
                   "pm_tsdf_integrate");
  return {{counts[0], counts[1]}};
}

std::array<int, 2> TsdfVolume::Integrate(const StereoModel& model, const Motion& pose, const core::Image<float>& disp,
                                         const core::Image<float>* weight, const TsdfIntegrateOptions& options) {
  if (disp.rows <= 0 || disp.cols <= 0) throw std::invalid_argument("TsdfVolume::Integrate: empty map");
  if (weight) SameSize(disp.rows, disp.cols, weight->rows, weight->cols, "TsdfVolume::Integrate");
  DeviceBuffers dev(impl_->h);
  const float* d_disp = dev.Put<float>(disp.data(), Bytes(disp));
  const float* d_weight = weight ? dev.Put<float>(weight->data(), Bytes(*weight)) : nullptr;
  return IntegrateDevice(model, pose, d_disp, d_weight, disp.rows, disp.cols, options,
                         /*want_counts=*/true);  // synchronises: the buffers may go
}

int TsdfVolume::RaycastDevice(const StereoModel& model, const Motion& pose, int rows, int cols, float* d_disp_out,
                              float* d_normals_out, const TsdfRaycastOptions& options, bool want_counts) {
  const pm_cloud_camera cam = CloudCamera(model);
  const pm_motion m = ToC(pose);
  const pm_tsdf_raycast_options opt = {options.min_range, options.max_range, options.step, options.min_weight};
  int hits = -1;
  impl_->dev.Check(pm_tsdf_raycast(impl_->h, &cam, &impl_->volume, &m, &opt, device(), rows, cols, d_disp_out, d_normals_out, nullptr,
                                   want_counts ? &hits : nullptr),
                   "pm_tsdf_raycast");
  return hits;
}

int TsdfVolume::Raycast(const StereoModel& model, const Motion& pose, int rows, int cols, core::Image<float>* disp,
                        core::Image<core::Vec3f>* normals, const TsdfRaycastOptions& options) {
  if (rows <= 0 || cols <= 0) throw std::invalid_argument("TsdfVolume::Raycast: empty size");
  const size_t px = (size_t)rows * cols;
  DeviceBuffers dev(impl_->h);
  float* d_disp = disp ? dev.Get<float>(4 * px) : nullptr;
  float* d_normals = normals ? dev.Get<float>(12 * px) : nullptr;
  const int hits = RaycastDevice(model, pose, rows, cols, d_disp, d_normals, options, /*want_counts=*/true);
  if (disp) dev.Fetch(disp, d_disp, rows, cols);
  if (normals) dev.Fetch(normals, d_normals, rows, cols);
  return hits;
}

Motion TsdfVolume::Align(const StereoModel& model, const Motion& pose_guess, const core::Image<float>& disp_new,
                         const TsdfRaycastOptions& raycast_options, const AlignOptions& align_options, pm_align_info* info) {
  const int rows = disp_new.rows, cols = disp_new.cols;
  if (rows <= 0 || cols <= 0) throw std::invalid_argument("TsdfVolume::Align: empty map");
  const size_t px = (size_t)rows * cols;
  Impl& m = *impl_;
  if (px > m.align_px) {
    m.align_disp = m.dev.Get<float>(4 * px);
    m.align_normals = m.dev.Get<float>(12 * px);
    m.align_new = m.dev.Get<float>(4 * px);
    m.align_px = px;
  }
  m.dev.Check(pm_upload(m.h, m.align_new, disp_new.data(), Bytes(disp_new)), "pm_upload");
  RaycastDevice(model, pose_guess, rows, cols, m.align_disp, m.align_normals, raycast_options, /*want_counts=*/false);
  const pm_cloud_camera cam = CloudCamera(model);
  const pm_align_options opt = ToC(align_options);
  pm_motion out;
  pm_align_info local;
  pm_align_info* const report = info ? info : &local;
  m.dev.Check(pm_align_disparity(m.h, &cam, &opt, nullptr, m.align_disp, m.align_normals, m.align_new, rows, cols, &out, report),
              "pm_align_disparity");
  return report->valid ? ComposeMotion(FromC(out), pose_guess) : pose_guess;
}

namespace {
// TsdfVolume::AlignColor behind its two signatures: the render, its colour and the new frame live in buffers of this call.
template <typename Pixel>
Motion AlignColorVolume(TsdfVolume& v, pm_handle* h, const StereoModel& model, const Motion& pose_guess,
                        const core::Image<float>& disp_new, const core::Image<Pixel>& bgr_new,
                        const TsdfRaycastOptions& raycast_options, const AlignColorOptions& align_options,
                        const TsdfColorSampleOptions& color_options, pm_align_color_info* info) {
  const char* const who = "TsdfVolume::AlignColor";
  NeedColor(v, who);
  const int rows = disp_new.rows, cols = disp_new.cols;
  if (rows <= 0 || cols <= 0) throw std::invalid_argument("TsdfVolume::AlignColor: empty map");
  SameSize(rows, cols, bgr_new.rows, bgr_new.cols, who);
  const size_t px = (size_t)rows * cols;
  DeviceBuffers dev(h);
  float* d_disp = dev.Get<float>(4 * px);
  float* d_normals = dev.Get<float>(12 * px);
  float* d_bgr = dev.Get<float>(12 * px);
  const float* d_new = dev.Put<float>(disp_new.data(), Bytes(disp_new));
  const NewImage image(dev, bgr_new);
  v.RaycastDevice(model, pose_guess, rows, cols, d_disp, d_normals, raycast_options, /*want_counts=*/false);
  v.ColorMapDevice(model, pose_guess, d_disp, rows, cols, d_bgr, nullptr, color_options, /*want_counts=*/false);
  const pm_cloud_camera cam = CloudCamera(model);
  const pm_align_color_options opt = ToC(align_options);
  pm_motion out;
  pm_align_color_info local;
  pm_align_color_info* const report = info ? info : &local;
  dev.Check(pm_align_color_disparity(h, &cam, &opt, nullptr, d_disp, d_normals, d_bgr, d_new, image.bgr8, image.bgr, rows, cols, &out,
                                     report),
            "pm_align_color_disparity");  // synchronises: the buffers may go
  return report->geo.valid ? ComposeMotion(FromC(out), pose_guess) : pose_guess;
}
}  // namespace

Motion TsdfVolume::AlignColor(const StereoModel& model, const Motion& pose_guess, const core::Image<float>& disp_new,
                              const core::Image<core::Vec3b>& bgr_new, const TsdfRaycastOptions& raycast_options,
                              const AlignColorOptions& align_options, const TsdfColorSampleOptions& color_options,
                              pm_align_color_info* info) {
  return AlignColorVolume(*this, impl_->h, model, pose_guess, disp_new, bgr_new, raycast_options, align_options, color_options, info);
}

Motion TsdfVolume::AlignColor(const StereoModel& model, const Motion& pose_guess, const core::Image<float>& disp_new,
                              const core::Image<core::Vec3f>& bgr_new, const TsdfRaycastOptions& raycast_options,
                              const AlignColorOptions& align_options, const TsdfColorSampleOptions& color_options,
                              pm_align_color_info* info) {
  return AlignColorVolume(*this, impl_->h, model, pose_guess, disp_new, bgr_new, raycast_options, align_options, color_options, info);
}

std::array<int, 2> TsdfVolume::MeshDevice(const TsdfMeshOptions& options, int vertex_capacity, int tri_capacity, float* d_xyz_out,
                                          float* d_normals_out, int32_t* d_tri_out, int* d_counts, bool want_counts) {
  const pm_tsdf_mesh_options opt = {options.min_weight};
  int counts[2] = {-1, -1};
  impl_->dev.Check(pm_tsdf_mesh(impl_->h, &impl_->volume, &opt, device(), vertex_capacity, tri_capacity, d_xyz_out, d_normals_out,
                                d_tri_out, d_counts, want_counts ? counts : nullptr),
                   "pm_tsdf_mesh");
  return {{counts[0], counts[1]}};
}

TriangleMesh TsdfVolume::Mesh(const TsdfMeshOptions& options, bool want_normals, bool want_color,
                              const TsdfColorSampleOptions& color_options) {
  if (want_color) NeedColor(*this, "TsdfVolume::Mesh");
  // count first (both capacities 0), then outputs of exactly that size
  const std::array<int, 2> counts = MeshDevice(options, 0, 0, nullptr, nullptr, nullptr);
  TriangleMesh mesh;
  if (counts[0] <= 0) return mesh;
  const size_t n = (size_t)counts[0], t = (size_t)(counts[1] > 0 ? counts[1] : 0);
  DeviceBuffers dev(impl_->h);
  float* d_xyz = dev.Get<float>(n * sizeof(core::Vec3f));
  float* d_normals = want_normals ? dev.Get<float>(n * sizeof(core::Vec3f)) : nullptr;
  int32_t* d_tris = t ? dev.Get<int32_t>(t * 3 * sizeof(int32_t)) : nullptr;
  if (MeshDevice(options, counts[0], counts[1], d_xyz, d_normals, d_tris) != counts)
    throw std::runtime_error("TsdfVolume::Mesh: the counts changed between two passes over one volume");
  if (want_color) {  // on the device, directly behind the mesh
    uint8_t* d_bgr8 = dev.Get<uint8_t>(n * sizeof(core::Vec3b));
    const pm_tsdf_color_sample_options opt = {color_options.min_weight, color_options.byte_scale};
    dev.Check(pm_tsdf_color_points(impl_->h, &impl_->volume, &opt, color_device(), d_xyz, counts[0], nullptr, nullptr, d_bgr8, nullptr,
                                   nullptr),
              "pm_tsdf_color_points");
    mesh.vertices.bgr.resize(n);
    dev.Check(pm_download(impl_->h, mesh.vertices.bgr.data(), d_bgr8, n * sizeof(core::Vec3b)), "pm_download");
  }
  mesh.vertices.xyz.resize(n);
  dev.Check(pm_download(impl_->h, mesh.vertices.xyz.data(), d_xyz, n * sizeof(core::Vec3f)), "pm_download");
  if (want_normals) {
    mesh.vertices.normals.resize(n);
    dev.Check(pm_download(impl_->h, mesh.vertices.normals.data(), d_normals, n * sizeof(core::Vec3f)), "pm_download");
  }
  mesh.triangles.resize(t);
  if (t) dev.Check(pm_download(impl_->h, mesh.triangles.data(), d_tris, t * 3 * sizeof(int32_t)), "pm_download");
  return mesh;
}

std::vector<float> TsdfVolume::Download() {
  std::vector<float> out(2 * voxels());
  impl_->dev.Check(pm_download(impl_->h, out.data(), device(), sizeof(float) * out.size()), "pm_download");
  return out;
}

}  // namespace imaging
}  // namespace bm
