// tests/cpp/test_bicubic_local_mirror.cpp -- the C++ host mirror's Bicubic<T>::pchip / akima / hermite
// (ndarray-interp_amd/host/ndarray_interp.hpp): the refusals that need no device, then -- with a device -- one build of each
// and the node values back; without one the build must fail loudly.  Exit code 0 and "OK" on success.
#include <cstdio>
#include <cstring>
#include <string>

#include "../../ndarray-interp_amd/host/ndarray_interp.hpp"

using namespace ndarray_interp;

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);            \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

template <class F>
static std::string builder_error(F f, int kind) {
  try {
    f();
  } catch (const BuilderError& e) {
    return e.kind == kind ? e.what() : std::string("other kind: ") + e.what();
  } catch (const std::exception& e) {
    return std::string("other exception: ") + e.what();
  }
  return "no exception";
}

int main() {
  Array<double> z25({2, 5}), z52({5, 2}), z22({2, 2}), z33({3, 3});
  for (size_t i = 0; i < z33.len(); ++i) z33[i] = double(i * i);
  // Akima needs 3 points per axis, Pchip and caller-given derivatives 2
  std::string m = builder_error([&] { Interp2DBuilder<double>::new_(z25).strategy(Bicubic<double>::akima()).build(); },
                                BuilderError::NotEnoughData);
  CHECK(m.find("The 0-dimension has not enough data") != std::string::npos && m.find("Reqired: 3") != std::string::npos);
  m = builder_error([&] { Interp2DBuilder<double>::new_(z52).strategy(Bicubic<double>::akima()).build(); },
                    BuilderError::NotEnoughData);
  CHECK(m.find("The 1-dimension has not enough data") != std::string::npos);
  CHECK(Bicubic<double>::pchip().MINIMUM_DATA_LENGHT() == 2 && Bicubic<double>::akima().MINIMUM_DATA_LENGHT() == 3);
  CHECK(Bicubic<double>::hermite(z22, z22, z22).MINIMUM_DATA_LENGHT() == 2);
  // the tables of the hermite constructor have the data's shape
  m = builder_error([&] { Interp2DBuilder<double>::new_(z25).strategy(Bicubic<double>::hermite(z25, z52, z25)).build(); },
                    BuilderError::ShapeError);
  CHECK(m.find("zy has wrong shape. Expected: [2, 5], got: [5, 2]") != std::string::npos);
  // the library's own refusals arrive as they are
  ndi_interp2d_desc d{};
  d.dtype = NDI_F64; d.memspace = NDI_MEM_HOST; d.nx = 2; d.ny = 5; d.lanes = 1; d.x_len = 2; d.y_len = 5;
  d.data = z25.data.data();
  ndi_interp2d* h = reinterpret_cast<ndi_interp2d*>(&d);
  CHECK(ndi_interp2d_create_bicubic_local(&d, NDI_AKIMA, &h) == NDI_NOT_ENOUGH_DATA && h == nullptr);
  CHECK(std::strstr(ndi_last_error_string(), "Bicubic (Akima) needs at least 3 data points on each axis (got 2 x 5)"));
  CHECK(ndi_interp2d_create_bicubic_local(&d, NDI_CUBIC_SPLINE, &h) == NDI_BAD_ARG);
  CHECK(ndi_interp2d_create_bicubic_hermite(&d, z25.data.data(), z25.data.data(), nullptr, &h) == NDI_BAD_ARG);
  CHECK(std::strstr(ndi_last_error_string(), "zxy is null"));

  auto run = [&](Bicubic<double> s, const Array<double>& z) {
    auto ip = Interp2DBuilder<double>::new_(z).strategy(std::move(s)).build();
    double xs[2] = {0.0, double(z.shape[0] - 1)}, ys[2] = {0.0, double(z.shape[1] - 1)}, out[2] = {-1.0, -1.0};
    ip.strategy->interp_array_into(ip, xs, ys, 2, out, 1);
    CHECK(out[0] == z[0] && out[1] == z[z.len() - 1]);      // the corners are nodes: exact
  };
  if (device_count() == 0) {
    try {
      run(Bicubic<double>::pchip(), z22);
      CHECK(!"a build without a device must fail");
    } catch (const DeviceError& e) {
      CHECK(std::strstr(e.what(), "no CPU fallback"));
    }
  } else {
    run(Bicubic<double>::pchip(), z22);
    run(Bicubic<double>::akima(), z33);
    run(Bicubic<double>::hermite(z33, z33, z33), z33);
  }
  if (failures == 0) std::puts("OK");
  return failures != 0;
}
