/*
 * rgb_segment_host.cpp -- the host-only half of the segment part of include/ra_gpu_wal.h: the file layout and the
 * index walk of a segment file (src/ra_log_segment.erl:1118-1138, 1197-1219), and the descriptor checks of a compaction
 * group, of a mem-table flush, of a batched read and of the snapshot calls.  No HIP here, so the file also builds on
 * its own under the sanitizers (tests/test_segment.py::test_segment_scan_under_sanitizers,
 * tests/test_segment_compact.py::test_compact_descriptors_under_sanitizers,
 * tests/test_segment_compact_groups.py::test_plan_helpers_under_sanitizers,
 * tests/test_segment_flush.py::test_flush_descriptors_under_sanitizers,
 * tests/test_segment_read.py::test_read_descriptors_under_sanitizers,
 * tests/test_snapshot_files.py::test_snapshot_descriptors_under_sanitizers).
 */
#include <stdint.h>
#include "../../include/ra_gpu_wal.h"

extern "C" uint64_t rgb_segment_layout(const rgb_seg_entry *entries, uint32_t n, uint32_t max_count,
                                       uint64_t *out_offsets) {
  uint64_t pos = (uint64_t)RGB_SEG_HEADER_BYTES + (uint64_t)RGB_SEG_RECORD_BYTES * max_count;   /* data_start, :247 */
  for (uint32_t i = 0; i < n; ++i) {
    if (out_offsets) out_offsets[i] = pos;
    pos += entries[i].data_len;                                   /* data_offset = DataOffset + Length, :277 */
  }
  return pos;
}

/* ---- compaction: the descriptors of a group, checked before anything is enqueued ------------------------
 * Library-internal (rgb_segment.hip calls it; not in the header).  `with_live` = 0: the slices are not looked at
 * (rgb_segment_info without a live list).  `limit_count`: the live indexes are counted -- asked[s] per source,
 * rank[i] = the number of live indexes of the same source in front of pair i, *max_count their sum -- and more than
 * 65535 of them is refused; without it the three outputs are not written. */
extern "C" int rgb_seg_compact_check(const rgb_seg_source *sources, uint32_t n_sources, const uint64_t *live,
                                     uint32_t n_live, uint64_t files_bytes, int with_live, int limit_count,
                                     uint32_t *asked, uint32_t *rank, uint64_t *sum_bytes, uint32_t *max_count) {
  if (n_sources > RGB_SEG_COMPACT_MAX_SOURCES || (n_sources && !sources) || (n_live && !live)) return RGB_E_INVAL;
  uint64_t sum = 0, total = 0;
  for (uint32_t s = 0; s < n_sources; ++s) {
    const rgb_seg_source &src = sources[s];
    if (src.offset > files_bytes || src.n_bytes > files_bytes - src.offset) return RGB_E_INVAL;
    if (sum + src.n_bytes < sum) return RGB_E_INVAL;
    sum += src.n_bytes;
    if (!with_live) continue;
    if (src.live_first > n_live || src.live_n > n_live - src.live_first) return RGB_E_INVAL;
    uint64_t in_source = 0;
    for (uint32_t k = 0; k < src.live_n; ++k) {
      const uint32_t i = src.live_first + k;
      const uint64_t first = live[2 * (uint64_t)i], last = live[2 * (uint64_t)i + 1];
      if (first > last) return RGB_E_INVAL;
      if (k) {
        const uint64_t prev_last = live[2 * (uint64_t)i - 1];
        if (first <= prev_last || first - prev_last < 2u) return RGB_E_INVAL;       /* ascending, not adjacent */
      }
      if (!limit_count) continue;
      const uint64_t count = last - first;                                          /* + 1, below */
      if (count >= 65535u || in_source + count + 1u > 65535u) return RGB_E_INVAL;
      rank[i] = (uint32_t)in_source;
      in_source += count + 1u;
    }
    if (limit_count) {
      asked[s] = (uint32_t)in_source;
      total += in_source;
      if (total > 65535u) return RGB_E_INVAL;
    }
  }
  if (sum_bytes) *sum_bytes = sum;
  if (limit_count) *max_count = (uint32_t)total;
  return RGB_OK;
}

extern "C" int rgb_segment_compact_bound(const rgb_seg_source *sources, uint32_t n_sources, const uint64_t *live,
                                         uint32_t n_live, uint64_t files_bytes, uint64_t *bound_out,
                                         uint32_t *max_count_out) {
  if (!bound_out || !max_count_out) return RGB_E_INVAL;
  uint32_t asked[RGB_SEG_COMPACT_MAX_SOURCES];
  uint32_t *rank = n_live ? new uint32_t[n_live] : nullptr;
  uint64_t sum = 0;
  uint32_t max_count = 0;
  const int rc = rgb_seg_compact_check(sources, n_sources, live, n_live, files_bytes, 1, 1, asked, rank, &sum, &max_count);
  delete[] rank;
  if (rc) return rc;
  const uint64_t head = (uint64_t)RGB_SEG_HEADER_BYTES + (uint64_t)RGB_SEG_RECORD_BYTES * max_count;
  if (sum + head < sum) return RGB_E_INVAL;
  *bound_out = head + sum;
  *max_count_out = max_count;
  return RGB_OK;
}

/* ---- major compaction for many members: the plan (pure), and the descriptors of the batched copy ---------- */

namespace {
/* pairs [first, first + n) of `live`: ascending, not adjacent, first <= last */
inline bool pairs_ok(const uint64_t *live, uint32_t first, uint32_t n) {
  for (uint32_t k = 0; k < n; ++k) {
    const uint64_t i = (uint64_t)first + k;
    const uint64_t a = live[2 * i], b = live[2 * i + 1];
    if (a > b) return false;
    if (k) {
      const uint64_t prev_last = live[2 * i - 1];
      if (a <= prev_last || a - prev_last < 2u) return false;
    }
  }
  return true;
}
/* the pairs of the slice that meet {lo, hi}: [*from, *to), by two binary searches */
inline void pairs_in(const uint64_t *live, uint32_t first, uint32_t n, uint64_t lo, uint64_t hi, uint32_t *from,
                     uint32_t *to) {
  uint32_t a = 0, b = n;                                 /* a = pairs whose last < lo */
  while (a < b) {
    const uint32_t mid = a + (b - a) / 2u;
    if (live[2 * ((uint64_t)first + mid) + 1] < lo) a = mid + 1u; else b = mid;
  }
  *from = a;
  b = n;                                                 /* a = pairs whose first <= hi (not below *from) */
  while (a < b) {
    const uint32_t mid = a + (b - a) / 2u;
    if (live[2 * ((uint64_t)first + mid)] <= hi) a = mid + 1u; else b = mid;
  }
  *to = a;
}
/* One pass of the fold over every member; write = false counts only.  -> the pairs the selections hold. */
uint64_t select_pass(const rgb_seg_member *members, uint32_t n_members, const uint64_t *segrefs, const uint64_t *live,
                     rgb_seg_pick *picks, uint64_t *live_out, bool write) {
  uint64_t n_out = 0;
  for (uint32_t m = 0; m < n_members; ++m) {
    const rgb_seg_member &mb = members[m];
    uint64_t ceiling = ~0ull;                            /* ra_seq:limit/2 so far: Live holds nothing above it */
    for (uint32_t k = 0; k < mb.segref_n; ++k) {
      const uint64_t r = (uint64_t)mb.segref_first + k;
      const uint64_t start = segrefs[2 * r], end = segrefs[2 * r + 1];
      const uint64_t top = end < ceiling ? end : ceiling;
      uint32_t from = 0, to = 0;
      if (start <= top) pairs_in(live, mb.live_first, mb.live_n, start, top, &from, &to);
      if (write) {
        rgb_seg_pick p{};
        p.live_first = (uint32_t)n_out; p.live_n = to - from;
        p.flags = to == from ? RGB_SEG_PICK_UNREFERENCED : 0u;
        for (uint32_t j = from; j < to; ++j) {
          const uint64_t i = (uint64_t)mb.live_first + j;
          const uint64_t a = live[2 * i] < start ? start : live[2 * i], b = live[2 * i + 1] > top ? top : live[2 * i + 1];
          live_out[2 * (n_out + (j - from))] = a;
          live_out[2 * (n_out + (j - from)) + 1] = b;
          const uint64_t len = b - a + 1u;               /* 0: the one range of 2^64 indexes */
          p.num_live = (len == 0u || p.num_live + len < p.num_live) ? ~0ull : p.num_live + len;
        }
        picks[r] = p;
      }
      n_out += to - from;
      if (to != from) ceiling = top;                     /* min(ceiling, End), and only behind a selection */
    }
  }
  return n_out;
}
}  // namespace

extern "C" int rgb_segment_compact_select(const rgb_seg_member *members, uint32_t n_members, const uint64_t *segrefs,
                                          uint32_t n_segrefs, const uint64_t *live, uint32_t n_live, rgb_seg_pick *picks,
                                          uint64_t *live_out, uint32_t live_out_cap, uint32_t *n_live_out) {
  if (!n_live_out || (n_members && !members) || (n_segrefs && !segrefs) || (n_live && !live)) return RGB_E_INVAL;
  const bool sizing = !picks && !live_out;
  uint64_t next = 0;                                     /* the first segref a later slice may name */
  for (uint32_t m = 0; m < n_members; ++m) {
    const rgb_seg_member &mb = members[m];
    if (mb.segref_first > n_segrefs || mb.segref_n > n_segrefs - mb.segref_first) return RGB_E_INVAL;
    if (mb.segref_first < next) return RGB_E_INVAL;
    next = (uint64_t)mb.segref_first + mb.segref_n;
    if (mb.live_first > n_live || mb.live_n > n_live - mb.live_first) return RGB_E_INVAL;
    if (!pairs_ok(live, mb.live_first, mb.live_n)) return RGB_E_INVAL;
  }
  const uint64_t need = select_pass(members, n_members, segrefs, live, nullptr, nullptr, false);
  if (need > 0xFFFFFFFFull) return RGB_E_INVAL;
  if (!sizing) {
    if (need > live_out_cap || (n_segrefs && !picks) || (need && !live_out)) return RGB_E_INVAL;
    (void)select_pass(members, n_members, segrefs, live, picks, live_out, true);
  }
  *n_live_out = (uint32_t)need;
  return RGB_OK;
}

extern "C" int rgb_segment_compact_take_groups(rgb_seg_take_member *members, uint32_t n_members, const rgb_seg_info *infos,
                                               const uint64_t *num_live, uint32_t n_sources, uint64_t max_count,
                                               uint64_t max_size, uint32_t *group_of) {
  if ((n_members && !members) || (n_sources && (!infos || !num_live || !group_of))) return RGB_E_INVAL;
  uint64_t next = 0;
  for (uint32_t m = 0; m < n_members; ++m) {
    if (members[m].src_first > n_sources || members[m].src_n > n_sources - members[m].src_first) return RGB_E_INVAL;
    if (members[m].src_first < next) return RGB_E_INVAL;
    next = (uint64_t)members[m].src_first + members[m].src_n;
  }
  for (uint32_t s = 0; s < n_sources; ++s) group_of[s] = RGB_SEG_GROUP_NONE;   /* (a source no member names stays so) */
  for (uint32_t m = 0; m < n_members; ++m) {
    rgb_seg_take_member &mb = members[m];
    uint32_t *of = group_of + mb.src_first;
    uint32_t groups = 0, in_group = 0;                   /* in_group: the length of take_group's accumulator */
    uint64_t cnt = max_count, size = max_size;           /* the budgets left */
    bool crash = false;
    uint32_t k = 0;
    while (k < mb.src_n && !crash) {
      const rgb_seg_info &in = infos[mb.src_first + k];
      const uint64_t nl = num_live[mb.src_first + k];
      /* NumLive / NumEnts < 0.5 orelse LiveSz / AllDataSz < 0.5, as integers: x / y < 0.5 iff 2 x < y for y > 0, which
       * is what the float division answers while x and y are below 2^53 (both conversions and the quotient's
       * comparison with 0.5 are then exact enough: 2 x and y are integers).  A negative AllDataSz (Sz < IdxSz) makes
       * the quotient <= 0. */
      bool compactable;
      if (in.num_entries == 0u) { crash = true; break; }
      if (nl < 0x8000000000000000ull && 2u * nl < (uint64_t)in.num_entries) {
        compactable = true;
      } else if (in.size == in.index_size) {
        crash = true; break;
      } else if (in.size < in.index_size) {
        compactable = true;
      } else {
        const uint64_t all = in.size - in.index_size;
        compactable = in.live_size < 0x8000000000000000ull && 2u * in.live_size < all;
      }
      if (compactable) {
        if (nl > cnt || in.live_size > size) {           /* MaxCnt - NumLive < 0 orelse MaxSz - LiveSz < 0 */
          if (in_group == 0u) { of[k++] = RGB_SEG_GROUP_NONE; continue; }
          groups += 1u; in_group = 0u; cnt = max_count; size = max_size;      /* the source stays for the next group */
          continue;
        }
        of[k++] = groups; in_group += 1u; cnt -= nl; size -= in.live_size;
      } else {
        of[k++] = RGB_SEG_GROUP_NONE;
        if (in_group) { groups += 1u; in_group = 0u; cnt = max_count; size = max_size; }
      }
    }
    if (in_group) groups += 1u;
    if (crash) {
      for (uint32_t j = 0; j < mb.src_n; ++j) of[j] = RGB_SEG_GROUP_NONE;
      groups = 0u;
    }
    mb.n_groups = groups;
    mb.status = crash ? RGB_SEG_TAKE_BADARITH : RGB_SEG_TAKE_OK;
  }
  return RGB_OK;
}

/* Library-internal (rgb_segment.hip calls it; not in the header): the descriptors of a batched compaction.  Per source
 * asked[s] = its live indexes and group_of_src[s] = its group (0xFFFFFFFF: none), per pair rank[i] as
 * rgb_seg_compact_check, per group max_counts[g]; *sum_bytes = the n_bytes of the sources that groups name
 * (saturating), *total_count = the live indexes of all groups.  Every output may be NULL.  with_out: the groups' out
 * ranges lie inside out_bytes and do not overlap (`order`: scratch of n_groups values for that, may be NULL without). */
extern "C" int rgb_seg_compact_groups_check(const rgb_seg_group *groups, uint32_t n_groups, const rgb_seg_source *sources,
                                            uint32_t n_sources, const uint64_t *live, uint32_t n_live, uint64_t files_bytes,
                                            int with_out, uint64_t out_bytes, uint32_t *order, uint32_t *asked,
                                            uint32_t *group_of_src, uint32_t *rank, uint32_t *max_counts,
                                            uint64_t *sum_bytes, uint64_t *total_count) {
  if ((n_groups && !groups) || (n_sources && !sources) || (n_live && !live)) return RGB_E_INVAL;
  if (with_out && n_groups && !order) return RGB_E_INVAL;
  if (group_of_src) for (uint32_t s = 0; s < n_sources; ++s) group_of_src[s] = 0xFFFFFFFFu;
  if (asked) for (uint32_t s = 0; s < n_sources; ++s) asked[s] = 0u;
  for (uint32_t s = 0; s < n_sources; ++s)               /* every source, named by a group or not: its header is read */
    if (sources[s].offset > files_bytes || sources[s].n_bytes > files_bytes - sources[s].offset) return RGB_E_INVAL;
  /* a pair's rank within its source is kept per pair: two named sources may share pairs only from the same first pair
   * on.  owner[i] = the live_first of the slice that reached pair i first (n_live: none yet). */
  struct owners {
    uint32_t *p;
    explicit owners(uint32_t n) : p(n ? new uint32_t[n] : nullptr) { for (uint32_t i = 0; i < n; ++i) p[i] = n; }
    ~owners() { delete[] p; }
  } owner(n_groups ? n_live : 0u);
  uint64_t next = 0, sum = 0, total = 0;
  for (uint32_t g = 0; g < n_groups; ++g) {
    const rgb_seg_group &gr = groups[g];
    if (gr.src_first > n_sources || gr.src_n > n_sources - gr.src_first) return RGB_E_INVAL;
    if (gr.src_n && gr.src_first < next) return RGB_E_INVAL;                  /* ascending and disjoint */
    if (gr.src_n) next = (uint64_t)gr.src_first + gr.src_n;
    if (with_out && (gr.out_offset > out_bytes || gr.out_bytes > out_bytes - gr.out_offset)) return RGB_E_INVAL;
    uint64_t in_group = 0;
    for (uint32_t q = 0; q < gr.src_n; ++q) {
      const uint32_t s = gr.src_first + q;
      const rgb_seg_source &src = sources[s];
      sum = sum + src.n_bytes < sum ? ~0ull : sum + src.n_bytes;
      if (src.live_first > n_live || src.live_n > n_live - src.live_first) return RGB_E_INVAL;
      if (!pairs_ok(live, src.live_first, src.live_n)) return RGB_E_INVAL;
      uint64_t in_source = 0;
      for (uint32_t k = 0; k < src.live_n; ++k) {
        const uint64_t i = (uint64_t)src.live_first + k;
        const uint64_t count = live[2 * i + 1] - live[2 * i];                 /* + 1, below */
        if (count >= 65535u || in_source + count + 1u > 65535u) return RGB_E_INVAL;
        if (owner.p[i] != n_live && owner.p[i] != src.live_first) return RGB_E_INVAL;
        owner.p[i] = src.live_first;
        if (rank) rank[i] = (uint32_t)in_source;
        in_source += count + 1u;
      }
      in_group += in_source;
      if (in_group > 65535u) return RGB_E_INVAL;
      if (asked) asked[s] = (uint32_t)in_source;
      if (group_of_src) group_of_src[s] = g;
    }
    if (max_counts) max_counts[g] = (uint32_t)in_group;
    total += in_group;
  }
  if (total > 0xFFFFFFFFull - 256u) return RGB_E_INVAL;
  if (with_out && n_groups) {
    /* no two non-empty out ranges meet: sorted by offset (a heap sort on the indexes: no allocation here) */
    const uint32_t n = n_groups;
    for (uint32_t g = 0; g < n; ++g) order[g] = g;
    auto less = [&](uint32_t a, uint32_t b) { return groups[a].out_offset < groups[b].out_offset; };
    auto sift = [&](uint32_t root, uint32_t end) {
      for (;;) {
        uint32_t child = 2u * root + 1u;
        if (child >= end) return;
        if (child + 1u < end && less(order[child], order[child + 1u])) child += 1u;
        if (!less(order[root], order[child])) return;
        const uint32_t t = order[root]; order[root] = order[child]; order[child] = t;
        root = child;
      }
    };
    for (uint32_t i = n / 2u; i-- > 0u;) sift(i, n);
    for (uint32_t end = n; end-- > 1u;) {
      const uint32_t t = order[0]; order[0] = order[end]; order[end] = t;
      sift(0u, end);
    }
    uint64_t behind = 0;                                 /* the end of the non-empty ranges so far */
    for (uint32_t k = 0; k < n; ++k) {
      const rgb_seg_group &gr = groups[order[k]];
      if (gr.out_bytes == 0u) continue;
      if (gr.out_offset < behind) return RGB_E_INVAL;
      behind = gr.out_offset + gr.out_bytes;
    }
  }
  if (sum_bytes) *sum_bytes = sum;
  if (total_count) *total_count = total;
  return RGB_OK;
}

extern "C" int rgb_segment_compact_groups_bound(rgb_seg_group *groups, uint32_t n_groups, const rgb_seg_source *sources,
                                                uint32_t n_sources, const uint64_t *live, uint32_t n_live,
                                                uint64_t files_bytes, uint64_t *total_out, uint32_t *max_counts) {
  if (!total_out) return RGB_E_INVAL;
  int rc = rgb_seg_compact_groups_check(groups, n_groups, sources, n_sources, live, n_live, files_bytes, 0, 0, nullptr,
                                        nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (rc) return rc;
  /* (the counts once more, so that nothing is written before every group has been accepted) */
  uint64_t pos = 0;
  for (int pass = 0; pass < 2; ++pass) {
    pos = 0;
    for (uint32_t g = 0; g < n_groups; ++g) {
      uint64_t count = 0, bytes = 0;
      for (uint32_t q = 0; q < groups[g].src_n; ++q) {
        const rgb_seg_source &src = sources[groups[g].src_first + q];
        for (uint32_t k = 0; k < src.live_n; ++k) {
          const uint64_t i = (uint64_t)src.live_first + k;
          count += live[2 * i + 1] - live[2 * i] + 1u;
        }
        if (bytes + src.n_bytes < bytes) return RGB_E_INVAL;
        bytes += src.n_bytes;
      }
      const uint64_t head = (uint64_t)RGB_SEG_HEADER_BYTES + (uint64_t)RGB_SEG_RECORD_BYTES * count;
      if (bytes + head < bytes || pos + (bytes + head) < pos) return RGB_E_INVAL;
      if (pass) {
        groups[g].out_offset = pos; groups[g].out_bytes = bytes + head;
        if (max_counts) max_counts[g] = (uint32_t)count;
      }
      pos += bytes + head;
    }
  }
  *total_out = pos;
  return RGB_OK;
}

/* ---- mem-table flush: the writers of a call, checked before anything is enqueued -------------------------
 * Library-internal (rgb_segment.hip calls it; not in the header).  *covered = the entries the slices name,
 * *longest = the longest slice. */
extern "C" int rgb_seg_flush_check(const rgb_seg_writer *writers, uint32_t n_writers, uint32_t n_entries,
                                   uint32_t *covered, uint32_t *longest) {
  if (n_writers && !writers) return RGB_E_INVAL;
  uint64_t next = 0, sum = 0;                                      /* the first entry a later slice may name */
  uint32_t top = 0;
  for (uint32_t w = 0; w < n_writers; ++w) {
    const rgb_seg_writer &d = writers[w];
    if (d.entry_first > n_entries || d.entry_n > n_entries - d.entry_first) return RGB_E_INVAL;
    if (d.entry_first < next) return RGB_E_INVAL;                  /* ascending and disjoint */
    next = (uint64_t)d.entry_first + d.entry_n;
    if (d.open_max_count < 1u || d.open_max_count > 65535u || d.open_count > d.open_max_count) return RGB_E_INVAL;
    if (d.open_count == 0u) {
      if (d.range_first != RGB_UNDEF || d.range_last != RGB_UNDEF) return RGB_E_INVAL;
    } else if (d.range_first == RGB_UNDEF || d.range_last == RGB_UNDEF || d.range_first > d.range_last) {
      return RGB_E_INVAL;
    }
    sum += d.entry_n;
    if (d.entry_n > top) top = d.entry_n;
  }
  if (covered) *covered = (uint32_t)sum;                           /* <= n_entries: the slices are disjoint */
  if (longest) *longest = top;
  return RGB_OK;
}

extern "C" int rgb_segment_flush_bound(const rgb_seg_writer *writers, uint32_t n_writers, uint32_t n_entries,
                                       uint64_t data_bytes, uint64_t *out_bound, uint32_t *pieces_bound) {
  if (!out_bound || !pieces_bound) return RGB_E_INVAL;
  const int rc = rgb_seg_flush_check(writers, n_writers, n_entries, nullptr, nullptr);
  if (rc) return rc;
  const uint64_t per_entry = (uint64_t)(RGB_SEG_RECORD_BYTES + RGB_SEG_HEADER_BYTES) * n_entries;
  if (data_bytes + per_entry < data_bytes) return RGB_E_INVAL;
  *out_bound = data_bytes + per_entry;
  *pieces_bound = n_entries;
  return RGB_OK;
}

/* ---- reading entries back: the sources of a call, checked before anything is enqueued ---------------------
 * Library-internal (rgb_segment.hip calls it; not in the header), shared by both forms.  *covered = the requests the
 * slices name, *sum_bytes = the sum of the sources' n_bytes (saturating), *out_bound = a size of `out` that always
 * suffices: the sum of req_n * n_bytes (saturating). */
extern "C" int rgb_seg_read_check(const rgb_seg_read_source *sources, uint32_t n_sources, uint64_t files_bytes,
                                  uint32_t n_req, uint32_t flags, uint32_t *covered, uint64_t *sum_bytes,
                                  uint64_t *out_bound) {
  if (n_sources > RGB_SEG_READ_MAX_SOURCES || (n_sources && !sources)) return RGB_E_INVAL;
  if (flags & ~(RGB_SEG_READ_VERIFY | RGB_SEG_READ_NO_DATA)) return RGB_E_INVAL;
  if ((flags & RGB_SEG_READ_VERIFY) && (flags & RGB_SEG_READ_NO_DATA)) return RGB_E_INVAL;
  uint64_t next = 0, named = 0, sum = 0, bound = 0;              /* next: the first request a later slice may name */
  for (uint32_t s = 0; s < n_sources; ++s) {
    const rgb_seg_read_source &src = sources[s];
    if (src.offset > files_bytes || src.n_bytes > files_bytes - src.offset) return RGB_E_INVAL;
    if (src.req_first > n_req || src.req_n > n_req - src.req_first) return RGB_E_INVAL;
    if (src.req_first < next) return RGB_E_INVAL;                  /* ascending and disjoint */
    next = (uint64_t)src.req_first + src.req_n;
    named += src.req_n;
    sum = sum + src.n_bytes < sum ? ~0ull : sum + src.n_bytes;
    const uint64_t most = src.req_n && src.n_bytes > ~0ull / src.req_n ? ~0ull : src.n_bytes * src.req_n;
    bound = bound + most < bound ? ~0ull : bound + most;
  }
  if (covered) *covered = (uint32_t)named;                         /* <= n_req: the slices are disjoint */
  if (sum_bytes) *sum_bytes = sum;
  if (out_bound) *out_bound = bound;
  return RGB_OK;
}

/* ---- snapshots and checkpoints: the descriptors of a call, checked before anything is enqueued -------------
 * Library-internal (rgb_segment.hip calls them; not in the header).  *sum_bytes = the bytes the call checksums
 * (saturating). */
#define RGB_SNAP_MAX_ITEMS 0x7FFFFFFFu

static inline bool snap_inside(uint64_t offset, uint64_t n_bytes, uint64_t buffer_bytes) {
  return offset <= buffer_bytes && n_bytes <= buffer_bytes - offset;
}
static inline uint64_t snap_sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }

extern "C" int rgb_snapshot_spans_check(const rgb_crc_span *spans, uint32_t n, uint64_t data_bytes, uint64_t *sum_bytes) {
  if (n > RGB_SNAP_MAX_ITEMS || (n && !spans)) return RGB_E_INVAL;
  uint64_t sum = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (!snap_inside(spans[i].offset, spans[i].n_bytes, data_bytes)) return RGB_E_INVAL;
    sum = snap_sat_add(sum, spans[i].n_bytes);
  }
  if (sum_bytes) *sum_bytes = sum;
  return RGB_OK;
}

/* the bytes of one image; 0 and *ok = false when the sum does not fit 64 bits */
static inline uint64_t snap_image_bytes(const rgb_snap_item &it, bool *ok) {
  const uint64_t head = it.kind == RGB_SNAP_KIND_SNAPSHOT ? RGB_SNAP_META_HEADER_BYTES : RGB_SNAP_HEADER_BYTES;
  const uint64_t size = head + it.meta_len + it.data_bytes;
  *ok = size >= it.data_bytes;
  return *ok ? size : 0u;
}

extern "C" uint64_t rgb_snapshot_layout(rgb_snap_item *items, uint32_t n, uint64_t base) {
  uint64_t pos = base;
  for (uint32_t i = 0; i < n; ++i) {
    bool ok;
    items[i].out_offset = pos;
    pos += snap_image_bytes(items[i], &ok);
  }
  return pos;
}

extern "C" int rgb_snapshot_build_check(const rgb_snap_item *items, uint32_t n, uint64_t data_bytes, uint64_t out_bytes,
                                        uint64_t *sum_bytes) {
  if (n > RGB_SNAP_MAX_ITEMS || (n && !items)) return RGB_E_INVAL;
  uint64_t sum = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const rgb_snap_item &it = items[i];
    if (it.kind != RGB_SNAP_KIND_SNAPSHOT && it.kind != RGB_SNAP_KIND_INDEXES) return RGB_E_INVAL;
    if (it.kind == RGB_SNAP_KIND_INDEXES && it.meta_len != 0u) return RGB_E_INVAL;
    if (!snap_inside(it.meta_offset, it.meta_len, data_bytes)) return RGB_E_INVAL;
    if (!snap_inside(it.data_offset, it.data_bytes, data_bytes)) return RGB_E_INVAL;
    bool ok;
    const uint64_t size = snap_image_bytes(it, &ok);
    if (!ok || !snap_inside(it.out_offset, size, out_bytes)) return RGB_E_INVAL;
    sum = snap_sat_add(sum, size);
  }
  if (sum_bytes) *sum_bytes = sum;
  return RGB_OK;
}

extern "C" int rgb_snapshot_files_check(const rgb_snap_file *files, uint32_t n, uint64_t files_bytes, uint64_t *sum_bytes) {
  if (n > RGB_SNAP_MAX_ITEMS || (n && !files)) return RGB_E_INVAL;
  uint64_t sum = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const rgb_snap_file &f = files[i];
    if (f.kind != RGB_SNAP_KIND_SNAPSHOT && f.kind != RGB_SNAP_KIND_INDEXES) return RGB_E_INVAL;
    if (f.flags & ~RGB_SNAP_META_ONLY) return RGB_E_INVAL;
    if (!snap_inside(f.offset, f.n_bytes, files_bytes)) return RGB_E_INVAL;
    if (!(f.flags & RGB_SNAP_META_ONLY)) sum = snap_sat_add(sum, f.n_bytes);
  }
  if (sum_bytes) *sum_bytes = sum;
  return RGB_OK;
}

namespace {
inline uint64_t seg_be(const unsigned char *p, int nbytes) {
  uint64_t v = 0;
  for (int k = 0; k < nbytes; ++k) v = (v << 8) | p[k];
  return v;
}
}  // namespace

extern "C" int rgb_segment_scan(const void *bytes, uint64_t n_bytes, rgb_seg_entry *out, uint32_t cap,
                                uint32_t *n_out, uint32_t *version_out, uint32_t *max_count_out, uint32_t *end) {
  if (!bytes || !n_out || !version_out || !max_count_out || !end) return RGB_E_INVAL;
  const unsigned char *b = (const unsigned char *)bytes;
  /* <<"RASG", Version:16, MaxCount:16>> when Version =< 2 (:1124-1133); formats exist for 1 and 2 (:1180-1189) */
  if (n_bytes < RGB_SEG_HEADER_BYTES || b[0] != 'R' || b[1] != 'A' || b[2] != 'S' || b[3] != 'G') return RGB_E_INVAL;
  const uint32_t version = (uint32_t)seg_be(b + 4, 2), max_count = (uint32_t)seg_be(b + 6, 2);
  if (version < 1u || version > RGB_SEG_VERSION) return RGB_E_INVAL;
  *version_out = version;
  *max_count_out = max_count;
  const uint32_t rec = version == 2u ? RGB_SEG_RECORD_BYTES : RGB_SEG_RECORD_BYTES_V1;
  const int off_bytes = version == 2u ? 8 : 4;
  const bool count_only = out == nullptr;
  uint32_t n = 0;
  *end = RGB_SEG_END_FULL;
  for (uint32_t k = 0; k < max_count; ++k) {
    const uint64_t pos = (uint64_t)RGB_SEG_HEADER_BYTES + (uint64_t)rec * k;
    if (pos + rec > n_bytes) { *end = RGB_SEG_END_TRUNCATED; break; }       /* decode_index_record/3's last clause */
    const unsigned char *p = b + pos;
    const uint64_t idx = seg_be(p, 8), term = seg_be(p + 8, 8), data_off = seg_be(p + 16, off_bytes);
    const uint32_t len = (uint32_t)seg_be(p + 16 + off_bytes, 4), crc = (uint32_t)seg_be(p + 20 + off_bytes, 4);
    if (idx == 0 && term == 0 && data_off == 0 && len == 0 && crc == 0) { *end = RGB_SEG_END_ZEROS; break; }
    if (data_off > n_bytes || len > n_bytes - data_off) { *end = RGB_SEG_END_TRUNCATED; break; }
    if (!count_only) {
      if (n == cap) { *end = RGB_SEG_END_CAP; break; }
      rgb_seg_entry &r = out[n];
      r.index = idx; r.term = term; r.data_offset = data_off; r.data_len = len; r.crc = crc;
    }
    n += 1;
  }
  *n_out = n;
  return RGB_OK;
}
