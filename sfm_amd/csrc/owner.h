// Ownership templates shared by every handle.  No HIP includes: the growth
// logic and the per-thread cache compile with a plain C++ compiler, so the
// host sanitizer program (tests/asan) runs them over malloc / free.  The two
// HIP memory policies, Stream and Event are in dev_mem.h.
#pragma once
#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <map>
#include <memory>
#include <utility>
#include <vector>

namespace sfm {

// Move-only owner of one allocation.  Mem supplies
//   static int alloc(void** p, size_t bytes)   (0 on success)
//   static void release(void* p)
//   static int drain(Stream s)                  (wait for the work on s; 0 on success)
//   using Stream = ...
template <typename Mem>
class Buf {
 public:
  Buf() = default;
  Buf(Buf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr, o.bytes_ = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, bytes_ = o.bytes_;
      o.p_ = nullptr, o.bytes_ = 0;
    }
    return *this;
  }
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { reset(); }

  // Room for `need` bytes; the contents are DROPPED when it grows.  A buffer
  // that has to grow first waits for `drain` (non-null: the stream whose
  // work may still use the old allocation), releases, then allocates `want`
  // (>= need) bytes.  Non-zero (Mem::alloc's code) on failure, the buffer
  // then empty.
  int reserve(size_t need, size_t want, typename Mem::Stream drain) {
    if (bytes_ >= need) return 0;
    if (drain && p_) (void)Mem::drain(drain);
    reset();
    void* q = nullptr;
    const int rc = Mem::alloc(&q, want);
    if (rc) return rc;
    p_ = q, bytes_ = want;
    return 0;
  }
  void reset() {
    if (p_) Mem::release(p_);
    p_ = nullptr, bytes_ = 0;
  }
  size_t bytes() const { return bytes_; }
  void* get() const { return p_; }
  template <typename T>
  T* as() const { return static_cast<T*>(p_); }

 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
};

// K columns that grow as one table (the map store's): one n and one cap, in
// rows, and each column's bytes per row.  reserve() is the one keeper of
// contents: it allocates EVERY new column first; if one allocation fails it
// releases the new ones and returns Mem::alloc's code with the table as it
// was (pointers, n, cap, contents).  Only then are the n live rows copied on
// the stream, the stream drained and the columns swapped.  Growth: at least
// the need, at least double, at least 1024 rows.  Rows past n are the caller's
// to write and count after commit().  Beside Buf's hooks, Mem supplies
//   static int copy(void* dst, const void* src, size_t bytes, Stream s)   (enqueued on s)
template <typename Mem, int K>
class RowTable {
 public:
  explicit RowTable(std::array<size_t, K> width) : width_(width) {}
  RowTable(const RowTable&) = delete;
  RowTable& operator=(const RowTable&) = delete;
  ~RowTable() {
    for (void* p : col_)
      if (p) Mem::release(p);
  }
  int reserve(int64_t rows, typename Mem::Stream s) {
    if (rows <= cap_) return 0;
    const int64_t cap = std::max<int64_t>({rows, 2 * cap_, 1024});
    std::array<void*, K> fresh{};
    for (int c = 0; c < K; ++c)
      if (const int rc = Mem::alloc(&fresh[c], size_t(cap) * width_[c])) {
        while (c-- > 0) Mem::release(fresh[c]);
        return rc;
      }
    for (int c = 0; c < K && n_; ++c) (void)Mem::copy(fresh[c], col_[c], size_t(n_) * width_[c], s);
    if (cap_) (void)Mem::drain(s);
    for (int c = 0; c < K; ++c)
      if (col_[c]) Mem::release(col_[c]);
    col_ = fresh, cap_ = cap;
    return 0;
  }
  void commit(int64_t rows) { n_ += rows; }   // the rows written at n() .. n() + rows now count
  void truncate(int64_t rows) { n_ = rows; }  // the first `rows` (<= n()) stay
  int64_t n() const { return n_; }
  int64_t cap() const { return cap_; }
  template <typename T>
  T* col(int c) const { return static_cast<T*>(col_[c]); }

 private:
  std::array<size_t, K> width_;
  std::array<void*, K> col_{};
  int64_t n_ = 0, cap_ = 0;
};

// Allocations re-used by size across problems (the bundle adjuster's): the
// resident problem's, the running set-up's scratch, and a free list, whose
// smallest buffer of at least the request take() prefers if it is at most
// twice that (among equals the one retired first).  A buffer enters the free
// list only against a Drained, made by waiting for every stream that may
// still touch it; scratch that nobody waited for stays scratch.
template <typename Mem>
class Pool {
 public:
  struct Drained {
    int rc = 0;  // the first failed wait's code (Mem::drain's)
    Drained(std::initializer_list<typename Mem::Stream> streams) {
      for (auto s : streams)
        if (const int e = s ? Mem::drain(s) : 0) rc = rc ? rc : e;
    }
  };
  Pool() = default;
  Pool(const Pool&) = delete;
  Pool& operator=(const Pool&) = delete;
  ~Pool() { retire(resident_), retire(scratch_), trim(); }
  // `count` T (0 counts as 1) in a multiple of 256 bytes, contents undefined; Mem::alloc's code on failure
  template <typename T>
  int take(T** p, size_t count, bool scratch) {
    if (count == 0) count = 1;
    std::pair<size_t, void*> a((count * sizeof(T) + 255) & ~size_t(255), nullptr);  // (capacity, buffer)
    auto it = free_.lower_bound(a.first);
    if (it != free_.end() && it->first <= 2 * a.first) {
      a = *it;  // (with its true capacity)
      free_.erase(it);
    } else if (const int rc = Mem::alloc(&a.second, a.first)) {
      return rc;
    }
    (scratch ? scratch_ : resident_).push_back(a);
    *p = static_cast<T*>(a.second);
    return 0;
  }
  void retire_scratch(const Drained&) { retire(scratch_); }
  void retire_all(const Drained&) { retire(resident_), retire(scratch_); }
  void trim() {  // releases the free list
    for (auto& kv : free_) Mem::release(kv.second);
    free_.clear();
  }

 private:
  void retire(std::vector<std::pair<size_t, void*>>& l) {
    for (auto& a : l) free_.insert(a);  // (behind its equals: first retired, first out)
    l.clear();
  }
  std::vector<std::pair<size_t, void*>> resident_, scratch_;
  std::multimap<size_t, void*> free_;
};

// The calling thread's context for `key` (the device, or whatever else the
// context was made for), destroyed when the thread exits.  A context enters
// the cache only after its init(key) returned 0: after a failed init nothing
// is cached, *rc holds init's code, and the next call tries again.
template <typename Ctx, typename Key>
Ctx* thread_ctx(const Key& key, int* rc) {
  static thread_local std::map<Key, std::unique_ptr<Ctx>> cache;
  *rc = 0;
  auto it = cache.find(key);
  if (it != cache.end()) return it->second.get();
  std::unique_ptr<Ctx> c(new Ctx());
  *rc = c->init(key);
  if (*rc) return nullptr;
  return (cache[key] = std::move(c)).get();
}

}  // namespace sfm
