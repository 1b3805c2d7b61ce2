// Camera front end on the device: raw uint8 frames [B][im_h][im_w][3 or 4] with byte pitches -> the network's image, the reference's
// offline `downsample_im` (scripts/prepare_flow_im.py:18-26): skimage.transform.resize(order=1, anti_aliasing=False) by 1 / s where s
// divides the frame, the uint8 truncation and the row cutoff, then optionally the normalisation of crd_assemble_input.  One launch, no
// allocation, no synchronisation.  The arithmetic is integer up to the byte (include/camradepth_hip.h); the fp32 normalisation is
// k_assemble_input's expression, a division, a subtraction and a division, which nothing can contract.
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int PER = 8;                         // adjacent output pixels of one row per thread

struct Camera {
  const unsigned char* frames;
  long long row_pitch, frame_pitch;            // bytes
  int B, h, w, channels, s, y_cutoff, swap_rb, x_channels, groups;      // groups = ceil(w / PER) per output row
  unsigned char* image;                        // [B][h][w][3] or NULL
  float* x;                                    // [B][x_channels][h][w] or NULL
};

__device__ __forceinline__ float normalised(unsigned v, int k) {
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  return ((float)v / 255.f - mean[k]) / stdv[k];
}

// One pixel, any s, channel count and pitch: v[k] is the byte of the STORED channel k.
__device__ __forceinline__ void pixel(const Camera& a, const unsigned char* frame, int R, int c, unsigned (&v)[3]) {
  const int o = (a.s >> 1) - 1 + (a.s & 1);                      // even s: s / 2 - 1, the upper left of the four; odd s: s / 2, the centre
  const unsigned char* p0 = frame + (long long)(R * a.s + o) * a.row_pitch + (long long)(c * a.s + o) * a.channels;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int kk = a.swap_rb ? 2 - k : k;
    if (a.s & 1) {
      v[k] = p0[kk];
    } else {
      const unsigned char* p1 = p0 + a.row_pitch;
      v[k] = ((unsigned)p0[kk] + p0[a.channels + kk] + p1[kk] + p1[a.channels + kk]) >> 2;
    }
  }
}

__device__ __forceinline__ unsigned byte_of(const unsigned (&wd)[12], int i) { return (wd[i >> 2] >> (8 * (i & 3))) & 0xffu; }

// A thread makes PER adjacent pixels of output row r of frame b.  WIDE (s = 2, 3 channels, base and pitches multiples of 16, decided by
// the host): a whole group is 2 rows x 16 source pixels = 2 x 48 bytes from a 16-byte boundary, three 16-byte loads per row.  The row
// tail, and every group without WIDE, goes pixel by pixel; both make the same bytes.
template <bool WIDE>
__global__ __launch_bounds__(TPB) void k_camera_frontend(Camera a, long long n_items) {
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n_items; i += (long long)gridDim.x * TPB) {
    const int g = (int)(i % a.groups);
    const long long t = i / a.groups;
    const int r = (int)(t % a.h), b = (int)(t / a.h);
    const int c0 = g * PER, n = min(PER, a.w - c0), R = r + a.y_cutoff;
    const unsigned char* frame = a.frames + (long long)b * a.frame_pitch;
    unsigned v[PER][3];
    if (WIDE && n == PER) {
      unsigned top[12], bot[12];
      const uint4* p0 = reinterpret_cast<const uint4*>(frame + (long long)(2 * R) * a.row_pitch + (long long)c0 * 6);
      const uint4* p1 = reinterpret_cast<const uint4*>(frame + (long long)(2 * R + 1) * a.row_pitch + (long long)c0 * 6);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const uint4 u = p0[q], d = p1[q];
        top[4 * q] = u.x; top[4 * q + 1] = u.y; top[4 * q + 2] = u.z; top[4 * q + 3] = u.w;
        bot[4 * q] = d.x; bot[4 * q + 1] = d.y; bot[4 * q + 2] = d.z; bot[4 * q + 3] = d.w;
      }
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        unsigned src[3];
#pragma unroll
        for (int kk = 0; kk < 3; ++kk)
          src[kk] = (byte_of(top, 6 * j + kk) + byte_of(top, 6 * j + 3 + kk) + byte_of(bot, 6 * j + kk) + byte_of(bot, 6 * j + 3 + kk)) >> 2;
        v[j][0] = a.swap_rb ? src[2] : src[0];
        v[j][1] = src[1];
        v[j][2] = a.swap_rb ? src[0] : src[2];
      }
    } else {
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        v[j][0] = v[j][1] = v[j][2] = 0;
        if (j < n) pixel(a, frame, R, c0 + j, v[j]);
      }
    }
    const long long pix = ((long long)b * a.h + r) * a.w + c0;
    if (a.image) {
      unsigned char* dst = a.image + pix * 3;
      if (n == PER && (reinterpret_cast<uintptr_t>(dst) & 7) == 0) {
        unsigned o[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < PER; ++j)
#pragma unroll
          for (int k = 0; k < 3; ++k) o[(3 * j + k) >> 2] |= v[j][k] << (8 * ((3 * j + k) & 3));
        uint2* d2 = reinterpret_cast<uint2*>(dst);
        d2[0] = make_uint2(o[0], o[1]); d2[1] = make_uint2(o[2], o[3]); d2[2] = make_uint2(o[4], o[5]);
      } else {
#pragma unroll
        for (int j = 0; j < PER; ++j)
          if (j < n) { dst[3 * j] = (unsigned char)v[j][0]; dst[3 * j + 1] = (unsigned char)v[j][1]; dst[3 * j + 2] = (unsigned char)v[j][2]; }
      }
    }
    if (a.x) {
      const long long plane = (long long)a.h * a.w;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float* dst = a.x + ((long long)b * a.x_channels + k) * plane + (long long)r * a.w + c0;
        if (n == PER && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
          float4* d4 = reinterpret_cast<float4*>(dst);
          d4[0] = make_float4(normalised(v[0][k], k), normalised(v[1][k], k), normalised(v[2][k], k), normalised(v[3][k], k));
          d4[1] = make_float4(normalised(v[4][k], k), normalised(v[5][k], k), normalised(v[6][k], k), normalised(v[7][k], k));
        } else {
#pragma unroll
          for (int j = 0; j < PER; ++j)
            if (j < n) dst[j] = normalised(v[j][k], k);
        }
      }
    }
  }
}

inline bool aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

}  // namespace

extern "C" int crd_camera_frontend(const uint8_t* frames, int32_t B, int32_t im_h, int32_t im_w, int32_t channels, int64_t row_pitch,
                                   int64_t frame_pitch, int32_t swap_rb, int32_t downsample_scale, int32_t y_cutoff, uint8_t* image_u8,
                                   float* x, int32_t x_channels, crd_stream_t stream) {
  const int s = downsample_scale;
  CRD_CHECK_ARG(frames, "crd_camera_frontend: null pointer (frames)");
  CRD_CHECK_ARG(image_u8 || x, "crd_camera_frontend: null pointer (image_u8 and x: at least one output)");
  CRD_CHECK_ARG(B > 0 && im_h > 0 && im_w > 0, "crd_camera_frontend: bad argument (B %d, image %d x %d)", B, im_h, im_w);
  CRD_CHECK_ARG(channels == 3 || channels == 4, "crd_camera_frontend: bad argument (channels %d is neither 3 nor 4)", channels);
  CRD_CHECK_ARG(row_pitch >= (int64_t)im_w * channels, "crd_camera_frontend: bad argument (row_pitch %lld is less than the %lld bytes of a row)",
                (long long)row_pitch, (long long)im_w * channels);
  CRD_CHECK_ARG(frame_pitch / im_h >= row_pitch, "crd_camera_frontend: bad argument (frame_pitch %lld is less than %d rows of %lld bytes)",
                (long long)frame_pitch, im_h, (long long)row_pitch);
  CRD_CHECK_ARG(s >= 1 && s <= 4, "crd_camera_frontend: bad argument (downsample_scale %d outside 1 .. 4)", s);
  const int h_new = im_h / s, w_new = im_w / s;
  CRD_CHECK_ARG(y_cutoff >= 0 && y_cutoff < h_new, "crd_camera_frontend: bad argument (y_cutoff %d outside [0, %d))", y_cutoff, h_new);
  CRD_CHECK_ARG(!x || x_channels >= 3, "crd_camera_frontend: bad argument (x_channels %d: x holds at least the three image planes)", x_channels);
  CRD_CHECK_ARG(aligned(x, 4), "crd_camera_frontend: bad argument (x must be 4-byte aligned)");
  CRD_UNSUPPORTED(im_h % s == 0 && im_w % s == 0,
                  "crd_camera_frontend: unsupported (downsample_scale %d does not divide the image %d x %d: the zoom is then not 1 / s)", s,
                  im_h, im_w);
  Camera a;
  a.frames = frames; a.row_pitch = row_pitch; a.frame_pitch = frame_pitch; a.B = B; a.h = h_new - y_cutoff; a.w = w_new;
  a.channels = channels; a.s = s; a.y_cutoff = y_cutoff; a.swap_rb = swap_rb != 0; a.x_channels = x ? x_channels : 0;
  a.groups = (w_new + PER - 1) / PER; a.image = image_u8; a.x = x;
  const long long per = (long long)a.h * a.w, planes = (long long)B * (x && x_channels > 3 ? x_channels : 3);      // each below 2^62
  CRD_UNSUPPORTED(per <= 0x7fffffffll && planes <= 0x7fffffffll && per * planes <= 0x7fffffffll,
                  "crd_camera_frontend: unsupported (B %d, maps %d x %d, %d planes: beyond the 32-bit indices)", B, a.h, a.w,
                  x ? x_channels : 3);
  const long long n_items = (long long)B * a.h * a.groups;
  const bool wide = s == 2 && channels == 3 && aligned(frames, 16) && (row_pitch & 15) == 0 && (frame_pitch & 15) == 0;
  const dim3 grid(blocks_for(n_items, TPB, 1 << 20)), block(TPB);
  if (wide) hipLaunchKernelGGL(k_camera_frontend<true>, grid, block, 0, as_stream(stream), a, n_items);
  else hipLaunchKernelGGL(k_camera_frontend<false>, grid, block, 0, as_stream(stream), a, n_items);
  CRD_LAUNCH_CHECK("crd_camera_frontend");
  return CRD_OK;
}
