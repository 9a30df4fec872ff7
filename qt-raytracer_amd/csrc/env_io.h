// env_io.h — host-side helpers of the environment map (include/hippt.h hipptSetEnvironment):
// the texel-centre directions of the octahedral layout, the resampling of a lat-long image to it, and a
// PFM reader for the command-line tool.  No HIP: compiles with g++ alone (tests/native/env_io_check.cpp).
#pragma once

#include <string>
#include <vector>

namespace hippt {
namespace envio {

constexpr int kMaxEnvSize = 4096;
// A lat-long image's largest side (the reader's and the resampler's bound: 2^14 x 2^13 floats x 3 is 1.5 GiB).
constexpr int kMaxImageSide = 16384;

// The unit direction of the centre of texel (x, y) of a size x size map, in double.
void texel_direction(int size, int x, int y, double d[3]);

// dirs[3 (y size + x) ..]: the texel-centre directions, rounded to float.  size in 1..kMaxEnvSize.
void directions(int size, float *dirs);

// texels[3 (y size + x) ..]: the lat-long image rgb (width x height x 3, row 0 at +y; pixel (c, r)'s centre at
// theta = pi (r + 1/2) / height from +y, phi = 2 pi (c + 1/2) / width - pi, direction (sin theta cos phi,
// cos theta, sin theta sin phi)) sampled bilinearly, in double, at the texel-centre directions: wrapped in
// phi, clamped in theta.  False with a message for a null pointer or a size or dimension out of range.
bool from_equirect(const float *rgb, int width, int height, int size, float *texels, std::string *err);

// A colour PFM ("PF", width height, a negative scale: little-endian; rows bottom to top) as a lat-long image
// with row 0 on top.  False with a message for a file that cannot be opened, a malformed or truncated header,
// a grey ("Pf") or big-endian file, dimensions outside 1..kMaxImageSide, or short data.
bool read_pfm(const std::string &path, std::vector<float> &rgb, int &width, int &height, std::string *err);

}  // namespace envio
}  // namespace hippt
