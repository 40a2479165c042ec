// pm_head_plan.hpp -- the ONE launch that derives a head's planes from the prep kernel's output (pm_kernels.hpp::k_setup):
// its grid and what every block of it does, as pure functions.  No HIP header: host and device code compile it
// (tests/cpp/head_plan_main.cpp walks it with a host compiler alone; the launch is made from setup_grid and the kernel
// finds its work with setup_decode).  No choice made here changes a result.
//
// The launch is one linear grid of seven sections, in this order:
//   0 .. 3  the four transposes (u8 image, f32 gradient, u8 gradient, u16 packed), a 64 x 64 tile per block
//   4       the row triples, 5 the reference quads: 256 columns x kLinesPerSetupThread lines per block
//   6       the column triples: 32 lines x 64 rows per block
// Sections 4 .. 6 exist only where the handle has line planes (with_lines).  A block finds its section and its place
// (bx, by, z) there from the section sizes; z is a PLANE index (pair * 4 + plane) in the transposes and a SLOT index
// (pair * 2 + view) in the line sections.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PM_HEAD_HD __host__ __device__
#else
#define PM_HEAD_HD
#endif

namespace pm {

constexpr int kLinesPerSetupThread = 4;  // a thread of the row-triple / quad sections builds this many consecutive lines

struct SetupGrid {
  unsigned tx, ty, tz;  // transpose sections: (ceil(cols/64), ceil(rows/64), B * 4) each
  unsigned lx, ly, lz;  // row triples / quads: (ceil(cols/256), ceil(nrl / kLinesPerSetupThread), B * 2) each
  unsigned cx, cy, cz;  // column triples: (ceil(ncl/32), ceil(rows/64), B * 2)
  int with_lines;       // 0: transposes only (PM_SEM_GPU, plane mode, anchor engines)
  int view;             // -1: both views (tz = B * 4, lz = cz = B * 2); 0 / 1: that view's planes only (tz = B * 2, lz = cz = B)
};

// The grid for n pairs of rows x cols with nrl row lines and ncl column lines (PlaneSet::nrl / ncl); view as above.
inline SetupGrid setup_grid(int rows, int cols, int nrl, int ncl, int n, int view, int with_lines) {
  SetupGrid sg{};
  sg.view = view;
  sg.tx = (unsigned)((cols + 63) / 64);
  sg.ty = (unsigned)((rows + 63) / 64);
  sg.tz = (unsigned)(n * (view < 0 ? 4 : 2));
  sg.with_lines = with_lines ? 1 : 0;  // the line-triple / quad planes of the run engine (pm_run3.hpp)
  if (sg.with_lines) {
    sg.lx = (unsigned)((cols + 255) / 256);
    sg.ly = (unsigned)((nrl + kLinesPerSetupThread - 1) / kLinesPerSetupThread);
    sg.lz = (unsigned)(n * (view < 0 ? 2 : 1));
    sg.cx = (unsigned)((ncl + 31) / 32);
    sg.cy = (unsigned)((rows + 63) / 64);
    sg.cz = (unsigned)(n * (view < 0 ? 2 : 1));
  }
  return sg;
}

// blocks of a SetupGrid
PM_HEAD_HD inline unsigned setup_blocks(const SetupGrid& sg) {
  return 4 * sg.tx * sg.ty * sg.tz + (sg.with_lines ? 2 * sg.lx * sg.ly * sg.lz + sg.cx * sg.cy * sg.cz : 0);
}

enum SetupSection {
  kSetupTransposeImg8 = 0,
  kSetupTransposeG32 = 1,
  kSetupTransposeG8 = 2,
  kSetupTransposePk16 = 3,
  kSetupRowTriples = 4,
  kSetupQuads = 5,
  kSetupColTriples = 6,
  kSetupSections = 7,
};

// plane / slot indices of a one-view launch: planes 2 * view, 2 * view + 1 of every pair; slot = pair * 2 + view
PM_HEAD_HD inline int setup_plane_of(const SetupGrid& sg, int bz) {
  return sg.view < 0 ? bz : (bz >> 1) * 4 + 2 * sg.view + (bz & 1);
}
PM_HEAD_HD inline int setup_slot_of(const SetupGrid& sg, int z) { return sg.view < 0 ? z : z * 2 + sg.view; }

struct SetupBlock {
  int section;  // SetupSection
  int bx, by;   // the block's place in its section: by = tile row (transposes, column triples) or line group (4, 5)
  int z;        // plane index (sections 0 .. 3) or slot index (4 .. 6)
};

// What block b < setup_blocks(sg) of the launch does.
PM_HEAD_HD inline SetupBlock setup_decode(const SetupGrid& sg, unsigned b) {
  SetupBlock r;
  const unsigned nt = sg.tx * sg.ty * sg.tz;
  if (b < 4 * nt) {
    const unsigned kind = b / nt;
    b -= kind * nt;
    r.section = (int)kind;
    r.bx = (int)(b % sg.tx);
    r.by = (int)((b / sg.tx) % sg.ty);
    r.z = setup_plane_of(sg, (int)(b / (sg.tx * sg.ty)));
    return r;
  }
  b -= 4 * nt;
  const unsigned nl = sg.lx * sg.ly * sg.lz;
  if (b < 2 * nl) {
    r.section = b < nl ? kSetupRowTriples : kSetupQuads;
    if (b >= nl) b -= nl;
    r.bx = (int)(b % sg.lx);
    r.by = (int)((b / sg.lx) % sg.ly);
    r.z = setup_slot_of(sg, (int)(b / (sg.lx * sg.ly)));
    return r;
  }
  b -= 2 * nl;
  r.section = kSetupColTriples;
  r.bx = (int)(b % sg.cx);
  r.by = (int)((b / sg.cx) % sg.cy);
  r.z = setup_slot_of(sg, (int)(b / (sg.cx * sg.cy)));
  return r;
}

}  // namespace pm
