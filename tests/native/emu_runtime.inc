/* TEST INFRASTRUCTURE: the lane / block emulation behind tests/native/fake_hip (one definition per library:
 * kernel_on_cpu.cpp in a single-unit build, kernel_dispatch_on_cpu.cpp in the split build) */
thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;

/* ---- block emulation: one ucontext fiber per lane ------------------------------------------------ */
#include <ucontext.h>
#include <vector>
namespace emu {
namespace {
struct Fiber { ucontext_t ctx; char *stack; bool done; };
std::vector<Fiber> fibers;
ucontext_t sched_ctx;
int cur = -1;
const std::function<void()> *body_fn = nullptr;
unsigned char shfl_buf[1024][16];
constexpr size_t STACK = 512 * 1024;

/* ---- the schedule: in which order emu::launch runs the workgroups of a grid and the lanes of a workgroup ----------
 * A process-wide setting (emu_set_schedule below); the default is ascending / ascending.  On a device neither order is
 * defined: workgroups start and finish in any order, and between two barriers the wavefronts of a workgroup interleave
 * as the hardware likes.  The permuted modes let the CPU tests meet atomics that arrive out of index order.
 *
 * shfl, ballot and barrier need no change for this: a pass of the scheduler still runs EVERY live fiber exactly once up
 * to its next barrier, whatever the order inside the pass.  shfl / ballot write shfl_buf[own lane], wait for the end of
 * the pass (every slot is written by then), read shfl_buf[source lane], and wait once more before any slot can be
 * written again -- slots and the `done` flags are indexed by lane number, never by position in the pass. */
enum { ORDER_ASCENDING = 0, ORDER_DESCENDING = 1, ORDER_PERMUTED = 2, ORDER_WAVEFRONTS = 3, WAVE = 64 };
int block_mode = ORDER_ASCENDING, lane_mode = ORDER_ASCENDING;
unsigned long long rng_state = 0;
unsigned long long next_random() {                      /* splitmix64 */
  unsigned long long z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
/* ord[0 .. n) = the order in which 0 .. n-1 are run; `unit` > 1 permutes whole groups of `unit`, ascending inside */
void draw_order(std::vector<unsigned> &ord, unsigned n, int mode, unsigned unit) {
  ord.resize(n);
  for (unsigned i = 0; i < n; ++i) ord[i] = mode == ORDER_DESCENDING ? n - 1u - i : i;
  if (mode != ORDER_PERMUTED && mode != ORDER_WAVEFRONTS) return;
  if (mode == ORDER_PERMUTED) unit = 1u;
  const unsigned groups = (n + unit - 1u) / unit;
  std::vector<unsigned> g(groups);
  for (unsigned i = 0; i < groups; ++i) g[i] = i;
  for (unsigned i = groups; i > 1u; --i) {              /* Fisher-Yates */
    const unsigned j = (unsigned)(next_random() % i), t = g[i - 1u];
    g[i - 1u] = g[j]; g[j] = t;
  }
  unsigned k = 0;
  for (unsigned i = 0; i < groups; ++i)
    for (unsigned l = g[i] * unit; l < n && l < (g[i] + 1u) * unit; ++l) ord[k++] = l;
}
void entry() {
  (*body_fn)();
  fibers[cur].done = true;
  swapcontext(&fibers[cur].ctx, &sched_ctx);
}
}  // namespace
int lane() { return cur < 0 ? 0 : cur; }
void barrier() {
  if (cur < 0) return;                                  /* not inside a launch: single lane, nothing to wait for */
  swapcontext(&fibers[cur].ctx, &sched_ctx);
}
void shfl(void *value, size_t size, int src_lane) {
  if (cur < 0) return;
  memcpy(shfl_buf[cur], value, size);
  barrier();
  memcpy(value, shfl_buf[src_lane], size);
  barrier();
}
unsigned long long ballot(int pred) {
  if (cur < 0) return pred ? 1ull : 0ull;
  const unsigned char b = pred ? 1 : 0;
  memcpy(shfl_buf[cur], &b, 1);
  barrier();
  unsigned long long m = 0;
  for (unsigned i = 0; i < blockDim.x && i < 64; ++i)
    if (!fibers[i].done && shfl_buf[i][0]) m |= 1ull << i;
  barrier();
  return m;
}
void launch(dim3 grid, dim3 block, const std::function<void()> &body) {
  const unsigned nl = block.x;
  body_fn = &body;
  blockDim = block; gridDim = grid;
  if (fibers.size() < nl) {
    size_t old = fibers.size();
    fibers.resize(nl);
    for (size_t i = old; i < nl; ++i) fibers[i].stack = (char *)malloc(STACK);
  }
  std::vector<unsigned> block_ord, lane_ord;
  draw_order(block_ord, grid.x, block_mode, 1u);
  draw_order(lane_ord, nl, lane_mode, WAVE);
  for (unsigned bi = 0; bi < grid.x; ++bi) {
    const unsigned b = block_ord[bi];
    blockIdx = dim3(b);
    for (unsigned i = 0; i < nl; ++i) {
      getcontext(&fibers[i].ctx);
      fibers[i].ctx.uc_stack.ss_sp = fibers[i].stack;
      fibers[i].ctx.uc_stack.ss_size = STACK;
      fibers[i].ctx.uc_link = nullptr;
      fibers[i].done = false;
      makecontext(&fibers[i].ctx, entry, 0);
    }
    bool live = true;
    while (live) {                                      /* one pass = one barrier interval */
      live = false;
      if (lane_mode == ORDER_PERMUTED || lane_mode == ORDER_WAVEFRONTS)
        draw_order(lane_ord, nl, lane_mode, WAVE);        /* drawn anew for every barrier interval */
      for (unsigned li = 0; li < nl; ++li) {
        const unsigned i = lane_ord[li];
        if (fibers[i].done) continue;
        cur = (int)i;
        threadIdx = dim3(i);
        swapcontext(&sched_ctx, &fibers[i].ctx);
        live = live || !fibers[i].done;
      }
    }
  }
  cur = -1;
  body_fn = nullptr;
}
}  // namespace emu

/* The schedule of every later launch of this library: block_mode 0 ascending, 1 descending, 2 a permutation of
 * 0 .. grid.x-1 drawn per launch; lane_mode 0 ascending, 1 descending, 2 a permutation drawn anew for every barrier
 * interval, 3 "wavefronts" (the 64-lane groups permuted, ascending lanes inside each).  The draws come from one generator
 * that this call seeds.  -> the previous setting as block_mode | lane_mode << 8 (tests/emu_schedule.py refuses to set a
 * schedule over one that is not ascending), or -1 for a mode that does not exist (nothing changes). */
extern "C" int emu_set_schedule(int block_mode, int lane_mode, unsigned long long seed) {
  if (block_mode < 0 || block_mode > emu::ORDER_PERMUTED || lane_mode < 0 || lane_mode > emu::ORDER_WAVEFRONTS) return -1;
  const int prev = emu::block_mode | emu::lane_mode << 8;
  emu::block_mode = block_mode; emu::lane_mode = lane_mode;
  emu::rng_state = seed;
  return prev;
}
