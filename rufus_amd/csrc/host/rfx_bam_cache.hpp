// BAM-kind packed-read cache between `jellyfish count --bam CHR --keep-packed FILE X.bam` and `RUFUS.Filter --packed FILE
// .. X.bam ..`: the BAM twin of rfx_packed_cache.hpp.  Replaces the second and third inflate of the
// subject's file -- scripts/RunJellyForRUFUS.sh:28-29 reads all of X.bam for the count, runRufus.sh:964-967 reads it again
// (here: twice, a scan pass and a pull pass) for the read pull.  The count leaves the filter's view of every kept record
// and the record's ADDRESS; the filter scans the cache and inflates only the BGZF blocks that hold the records it wants.
//
// "The stream" is the concatenated inflated payload of ALL BGZF blocks of X.bam from byte 0, the BAM header included.
//
// The file (little endian, every part a multiple of 8 bytes):
//
//   FileHeader | names | chunk 0 | chunk 1 | ... | IndexHeader | IndexEntry[n_blocks] | FileHeader
//
//   FileHeader (96 bytes)  magic "RBAMCAC1"; min_q (the MinQ the `good` masks were made with); exclude_flags (records with
//       flag & exclude_flags are not in the cache); done ("CACHDONE" once the producer has finished, 0 before);
//       bam_bytes (the size of X.bam); stream_bytes; n_chunks; n_blocks; index_off (file offset of the IndexHeader);
//       n_records (all chunks' n); n_ref; names_bytes.  Written at the start without `done` (the totals still 0), and
//       again -- at the start AND behind the index -- when the count has seen the whole file.  A file whose two headers
//       differ, or lack `done`, is not a cache: its producer died, or it was cut.
//   names       the references' names as rfx_bam_header gives them: each with its NUL, one behind the other, names_bytes
//       bytes, padded to 8.
//   chunk       one per arena of the count that had kept records, in file order.  ChunkHeader (48 bytes): magic
//       "BMCHUNK1"; seq (0, 1, ...); stream_off (the stream offset of the arena's byte 0); bytes (of the whole chunk, its
//       header included); n (kept records); n_words; n_runs; 0.  Then, each padded to 8 bytes:
//         hash u64[n]        the QNAME hash of rfx_bam_core.h (FNV-1a, then the splitmix64 finaliser)
//         start u32[n]       the arena offset of the record's block_size field: the record is the stream's bytes
//         rbytes u32[n]      [stream_off + start, stream_off + start + rbytes), rbytes = 4 + block_size
//         len u32[n] | word_off u32[n + 1] | codes u64[n_words] | good u32[n_words]
//                            the filter block of the kept records as rfx_reads_get hands it out (rfx_bam_parse_filter)
//         runs u32[2 n_runs] (first kept index, refID) wherever a kept record's refID differs from its predecessor's
//       There is no "always" flag: the device packs every record exactly.
//   index       IndexHeader (16 bytes): magic "BMINDEX1", n_blocks.  IndexEntry (24 bytes) for every BGZF block of X.bam,
//       in order: file_off, inflated_off (the stream offset of its first byte), csize (its bytes in the file), isize.
//
// read_cache() checks everything the filter will index with; plan_fetch() turns selected records into batches of blocks
// that fit an arena.  Pure host code: no device call, no other project header.
#pragma once
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace rfxbamcache {

constexpr uint64_t FILE_MAGIC = 0x314341434D414252ull;   // "RBAMCAC1"
constexpr uint64_t CHUNK_MAGIC = 0x314B4E5548434D42ull;  // "BMCHUNK1"
constexpr uint64_t INDEX_MAGIC = 0x315845444E494D42ull;  // "BMINDEX1"
constexpr uint64_t DONE_MAGIC = 0x454E4F4448434143ull;   // "CACHDONE"
constexpr uint32_t RECORD_MIN = 36;                       // block_size + the fixed fields

struct FileHeader {
  uint64_t magic = FILE_MAGIC;
  int32_t min_q = 0;
  uint32_t exclude_flags = 0;
  uint64_t done = 0;
  uint64_t bam_bytes = 0, stream_bytes = 0;
  uint64_t n_chunks = 0, n_blocks = 0;
  uint64_t index_off = 0;
  uint64_t n_records = 0;
  uint32_t n_ref = 0, names_bytes = 0;
  uint64_t pad[2] = {0, 0};
};
static_assert(sizeof(FileHeader) == 96, "the file header is 96 bytes");

struct ChunkHeader {
  uint64_t magic = CHUNK_MAGIC;
  uint64_t seq = 0, stream_off = 0, bytes = 0;
  uint32_t n = 0, n_words = 0, n_runs = 0, reserved = 0;
};
static_assert(sizeof(ChunkHeader) == 48, "the chunk header is 48 bytes");

struct IndexHeader {
  uint64_t magic = INDEX_MAGIC;
  uint64_t n_blocks = 0;
};
struct IndexEntry {
  uint64_t file_off = 0, inflated_off = 0;
  uint32_t csize = 0, isize = 0;
};
static_assert(sizeof(IndexEntry) == 24, "an index entry is 24 bytes");

inline size_t pad8(size_t x) { return (x + 7) & ~(size_t)7; }

// A chunk as its producer or its reader holds it (pointers into the caller's arrays / the mapped file).
struct Chunk {
  uint64_t seq = 0, stream_off = 0;
  uint32_t n = 0, n_words = 0, n_runs = 0;
  const uint64_t* hash = nullptr;
  const uint32_t *start = nullptr, *rbytes = nullptr, *len = nullptr, *word_off = nullptr;
  const uint64_t* codes = nullptr;
  const uint32_t *good = nullptr, *runs = nullptr;
};

inline size_t chunk_bytes(uint32_t n, uint32_t n_words, uint32_t n_runs) {
  return sizeof(ChunkHeader) + (size_t)n * 8 + 3 * pad8((size_t)n * 4) + pad8(((size_t)n + 1) * 4) + (size_t)n_words * 8 +
         pad8((size_t)n_words * 4) + (size_t)n_runs * 8;
}

inline void serialize_chunk(const Chunk& c, std::vector<char>& out) {
  ChunkHeader h;
  h.seq = c.seq;
  h.stream_off = c.stream_off;
  h.n = c.n;
  h.n_words = c.n_words;
  h.n_runs = c.n_runs;
  h.bytes = chunk_bytes(c.n, c.n_words, c.n_runs);
  out.assign((size_t)h.bytes, 0);
  char* p = out.data();
  memcpy(p, &h, sizeof h);
  size_t o = sizeof h;
  auto put = [&](const void* src, size_t bytes, size_t padded) {
    if (bytes) memcpy(p + o, src, bytes);
    o += padded;
  };
  const size_t n = c.n, w = c.n_words;
  put(c.hash, n * 8, n * 8);
  put(c.start, n * 4, pad8(n * 4));
  put(c.rbytes, n * 4, pad8(n * 4));
  put(c.len, n * 4, pad8(n * 4));
  put(c.word_off, (n + 1) * 4, pad8((n + 1) * 4));
  put(c.codes, w * 8, w * 8);
  put(c.good, w * 4, pad8(w * 4));
  put(c.runs, (size_t)c.n_runs * 8, (size_t)c.n_runs * 8);
}

// The producer.  Every call returns false on a write error (errno says why): the count ends then -- a cache that silently
// lacks records is worse than none.
class Writer {
  int fd_ = -1;
  uint64_t at_ = 0;
  FileHeader h_;
  std::string names_;
  std::vector<IndexEntry> index_;
  std::vector<char> buf_;

  bool write_at(const void* p, size_t n, uint64_t at) {
    const char* b = (const char*)p;
    while (n) {
      const ssize_t w = ::pwrite(fd_, b, n, (off_t)at);
      if (w < 0 && errno == EINTR) continue;
      if (w <= 0) return false;
      b += w, n -= (size_t)w, at += (uint64_t)w;
    }
    return true;
  }
  bool append(const void* p, size_t n) {
    if (!write_at(p, n, at_)) return false;
    at_ += n;
    return true;
  }

 public:
  // names: each with its NUL, one behind the other (rfx_bam_header's)
  bool open(int fd, int min_q, uint32_t exclude_flags, uint32_t n_ref, const char* names, size_t names_bytes) {
    fd_ = fd;
    at_ = 0;
    h_ = FileHeader();
    h_.min_q = min_q;
    h_.exclude_flags = exclude_flags;
    h_.n_ref = n_ref;
    h_.names_bytes = (uint32_t)names_bytes;
    names_.assign(names ? names : "", names ? names_bytes : 0);
    names_.resize(pad8(names_bytes), '\0');
    index_.clear();
    return append(&h_, sizeof h_) && append(names_.data(), names_.size());
  }
  // c.seq is set here: chunks are numbered as they come
  bool add_chunk(Chunk c) {
    c.seq = h_.n_chunks;
    serialize_chunk(c, buf_);
    if (!append(buf_.data(), buf_.size())) return false;
    ++h_.n_chunks;
    h_.n_records += c.n;
    return true;
  }
  // the next BGZF block of the file, in file order
  void add_block(uint32_t csize, uint32_t isize) {
    IndexEntry e;
    e.file_off = h_.bam_bytes;
    e.inflated_off = h_.stream_bytes;
    e.csize = csize;
    e.isize = isize;
    index_.push_back(e);
    h_.bam_bytes += csize;
    h_.stream_bytes += isize;
  }
  uint64_t stream_bytes() const { return h_.stream_bytes; }
  uint64_t file_bytes() const { return at_; }
  uint64_t records() const { return h_.n_records; }
  // the index, and the header twice; the caller closes the descriptor (and checks that too)
  bool finish() {
    h_.n_blocks = index_.size();
    h_.index_off = at_;
    h_.done = DONE_MAGIC;
    IndexHeader ih;
    ih.n_blocks = index_.size();
    return append(&ih, sizeof ih) && append(index_.data(), index_.size() * sizeof(IndexEntry)) && append(&h_, sizeof h_) &&
           write_at(&h_, sizeof h_, 0);
  }
};

struct Cache {
  FileHeader h;
  std::vector<std::string> names;
  std::vector<Chunk> chunks;  // by seq
  const IndexEntry* index = nullptr;
};

// A mapped cache file -> its parts; false: not a BAM-kind cache, not finished, cut, or inconsistent in itself.  Everything
// the filter indexes with is checked here: chunk bounds inside the file, word_off monotone and inside the chunk's words,
// every record inside the stream, the block index contiguous from 0 to (bam_bytes, stream_bytes).  `base` must be aligned to
// 8 bytes (a mapping is).
inline bool read_cache(const char* base, size_t size, Cache& out) {
  out = Cache();
  if (((uintptr_t)base & 7u) || size < 2 * sizeof(FileHeader) || (size & 7u)) return false;
  FileHeader& h = out.h;
  memcpy(&h, base, sizeof h);
  if (h.magic != FILE_MAGIC || h.done != DONE_MAGIC) return false;
  if (memcmp(base, base + size - sizeof h, sizeof h) != 0) return false;  // the header behind the index
  // the index: exactly between index_off and the last header
  const size_t body_end = size - sizeof h;
  if (h.n_blocks > (size / sizeof(IndexEntry)) || h.index_off > body_end || (h.index_off & 7u)) return false;
  if (body_end - h.index_off != sizeof(IndexHeader) + h.n_blocks * sizeof(IndexEntry)) return false;
  IndexHeader ih;
  memcpy(&ih, base + h.index_off, sizeof ih);
  if (ih.magic != INDEX_MAGIC || ih.n_blocks != h.n_blocks) return false;
  out.index = (const IndexEntry*)(base + h.index_off + sizeof ih);
  uint64_t f = 0, s = 0;
  for (uint64_t i = 0; i < h.n_blocks; ++i) {
    const IndexEntry& e = out.index[i];
    if (e.file_off != f || e.inflated_off != s || e.csize == 0 || e.csize > 65536u || e.isize > 65536u) return false;
    f += e.csize;
    s += e.isize;
  }
  if (f != h.bam_bytes || s != h.stream_bytes) return false;
  // the names
  size_t at = sizeof h;
  if (h.names_bytes > h.index_off || at + pad8(h.names_bytes) > h.index_off) return false;
  {
    const char* p = base + at;
    size_t i = 0;
    while (i < h.names_bytes) {
      const void* nul = memchr(p + i, 0, h.names_bytes - i);
      if (!nul) return false;
      out.names.emplace_back(p + i, (const char*)nul);
      i = (size_t)((const char*)nul - p) + 1;
    }
    if (out.names.size() != h.n_ref) return false;
  }
  at += pad8(h.names_bytes);
  // the chunks: they fill the file up to the index
  uint64_t records = 0, last_end = 0;
  while (at < h.index_off) {
    if (h.index_off - at < sizeof(ChunkHeader)) return false;
    ChunkHeader ch;
    memcpy(&ch, base + at, sizeof ch);
    if (ch.magic != CHUNK_MAGIC || ch.seq != out.chunks.size() || ch.reserved != 0) return false;
    if (ch.bytes != chunk_bytes(ch.n, ch.n_words, ch.n_runs) || ch.bytes > h.index_off - at) return false;
    Chunk c;
    c.seq = ch.seq, c.stream_off = ch.stream_off, c.n = ch.n, c.n_words = ch.n_words, c.n_runs = ch.n_runs;
    const size_t n = ch.n, w = ch.n_words;
    size_t o = at + sizeof ch;
    c.hash = (const uint64_t*)(base + o); o += n * 8;
    c.start = (const uint32_t*)(base + o); o += pad8(n * 4);
    c.rbytes = (const uint32_t*)(base + o); o += pad8(n * 4);
    c.len = (const uint32_t*)(base + o); o += pad8(n * 4);
    c.word_off = (const uint32_t*)(base + o); o += pad8((n + 1) * 4);
    c.codes = (const uint64_t*)(base + o); o += w * 8;
    c.good = (const uint32_t*)(base + o); o += pad8(w * 4);
    c.runs = (const uint32_t*)(base + o); o += (size_t)ch.n_runs * 8;
    if (o != at + ch.bytes) return false;  // (cannot differ: chunk_bytes is this sum)
    if (n == 0 || ch.stream_off > h.stream_bytes) return false;  // (an arena without kept records leaves no chunk)
    if (c.word_off[0] != 0 || c.word_off[n] != w) return false;
    for (size_t r = 0; r < n; ++r) {
      if (c.word_off[r] > c.word_off[r + 1] || (uint64_t)(c.word_off[r + 1] - c.word_off[r]) * 32 < c.len[r]) return false;
      const uint64_t rs = ch.stream_off + c.start[r];
      if (c.rbytes[r] < RECORD_MIN || rs + c.rbytes[r] > h.stream_bytes) return false;
      if (rs < last_end) return false;  // the records lie one behind the other, in file order, across chunks too
      last_end = rs + c.rbytes[r];
    }
    if (ch.n_runs == 0 || ch.n_runs > n || c.runs[0] != 0) return false;
    for (size_t r = 0; r < ch.n_runs; ++r) {
      if (c.runs[2 * r] >= n || (r && c.runs[2 * r] <= c.runs[2 * r - 2])) return false;
      const int32_t ref = (int32_t)c.runs[2 * r + 1];
      if (ref < -1 || (ref >= 0 && (uint32_t)ref >= h.n_ref)) return false;
    }
    records += n;
    out.chunks.push_back(c);
    at += ch.bytes;
  }
  return out.chunks.size() == h.n_chunks && records == h.n_records;
}

// ---- the fetch plan ------------------------------------------------------------------------------------------------------
struct Selected {
  uint64_t stream_off = 0;  // of the record's block_size field
  uint32_t bytes = 0;
};
struct Batch {
  std::vector<uint64_t> block;      // indices into the index, ascending, each once
  uint64_t inflated = 0;            // what they inflate to, one behind the other: <= the capacity
  size_t first = 0, n = 0;          // the batch's records: sel[first, first + n)
  std::vector<uint32_t> arena_off;  // n of them: where record first + i begins in the concatenated inflated blocks
};

// the block that holds stream byte `off` (< stream_bytes): the last one that starts at or in front of it -- blocks of
// ISIZE 0 start where their successor starts and never are the last such
inline uint64_t block_of(const IndexEntry* index, uint64_t n_blocks, uint64_t off) {
  uint64_t lo = 0, hi = n_blocks;  // index[lo].inflated_off <= off (index[0].inflated_off = 0)
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (index[mid].inflated_off <= off) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Batches for the selected records, which come ascending by stream offset (equal and overlapping ranges are allowed) and
// are not reordered.  A batch's blocks are the blocks (of ISIZE > 0) that overlap any of its records' byte ranges, each
// once, in file order; all blocks of one record lie in one batch and -- every block between a record's first and last
// being one of them -- side by side in the arena.  A batch's inflated total is <= capacity; a block shared by the last
// record of one batch and the first of the next is listed in both.  false with *err set: a record outside the stream,
// records not ascending, a record whose blocks alone exceed the capacity.
inline bool plan_fetch(const IndexEntry* index, uint64_t n_blocks, uint64_t stream_bytes, const std::vector<Selected>& sel,
                       uint64_t capacity, std::vector<Batch>& out, std::string* err) {
  out.clear();
  auto fail = [&](size_t i, const char* what) {
    if (err) *err = "record " + std::to_string(i) + ": " + what;
    out.clear();
    return false;
  };
  capacity = std::min<uint64_t>(capacity, 0xFFFFFFFFull);  // (arena offsets are 32 bits)
  if (n_blocks == 0 && !sel.empty()) return fail(0, "outside the stream");
  uint64_t last_block = 0;  // of the open batch
  for (size_t i = 0; i < sel.size(); ++i) {
    const Selected& s = sel[i];
    if (s.bytes == 0 || s.stream_off >= stream_bytes || stream_bytes - s.stream_off < s.bytes) return fail(i, "outside the stream");
    if (i && s.stream_off < sel[i - 1].stream_off) return fail(i, "not ascending");
    const uint64_t fb = block_of(index, n_blocks, s.stream_off), lb = block_of(index, n_blocks, s.stream_off + s.bytes - 1);
    const uint64_t own = index[lb].inflated_off + index[lb].isize - index[fb].inflated_off;  // its blocks' inflated bytes
    if (own > capacity) return fail(i, "its blocks exceed the arena");
    bool fresh = out.empty();
    if (!fresh) {
      // what the record adds to the open batch: its blocks behind the batch's last (fb >= the batch's first: ascending)
      const uint64_t from = std::max(fb, last_block + 1);
      const uint64_t add = lb >= from ? index[lb].inflated_off + index[lb].isize - index[from].inflated_off : 0;
      if (out.back().inflated + add > capacity) fresh = true;
    }
    if (fresh) {
      out.emplace_back();
      out.back().first = i;
    }
    Batch& b = out.back();
    uint64_t at_fb = 0;  // fb's place in the batch's arena
    bool have_fb = false;
    for (uint64_t k = (fresh ? fb : std::max(fb, last_block + 1)); k <= lb; ++k) {
      if (index[k].isize == 0) continue;
      if (k == fb) at_fb = b.inflated, have_fb = true;
      b.block.push_back(k);
      b.inflated += index[k].isize;
    }
    if (!have_fb) {  // fb came with an earlier record of the batch: the inflated bytes of the batch's blocks in front of it
      at_fb = 0;
      for (size_t j = b.block.size(); j-- > 0;) {
        if (b.block[j] == fb) {
          at_fb = b.inflated;
          for (size_t t = j; t < b.block.size(); ++t) at_fb -= index[b.block[t]].isize;
          have_fb = true;
          break;
        }
        if (b.block[j] < fb) break;
      }
      if (!have_fb) return fail(i, "its first block is not in the batch");  // (cannot be)
    }
    b.arena_off.push_back((uint32_t)(at_fb + (s.stream_off - index[fb].inflated_off)));
    ++b.n;
    last_block = b.block.empty() ? last_block : b.block.back();
  }
  return true;
}

}  // namespace rfxbamcache
