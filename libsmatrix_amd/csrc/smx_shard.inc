// smx_shard.inc -- the multi-GPU router INSIDE the C library (include/smatrix_shard.h, "router" section).
// Included by smx_runtime.hip.  No reference counterpart: the reference is one process (SURVEY.md 8e).
//
// One process per GPU; rank r owns the rows whose owner_of(x) == r and keeps them in an ordinary smatrix_t.
// A batch submitted on every rank (collectively, each rank its own n) is
//   1. partitioned by owner on the GPU into one packed {x,y[,v]} record per op (k_part_count / k_part_scatter),
//   2. exchanged: per-peer counts first (8 bytes per pair), then the records -- an alltoallv,
//   3. applied by the owner IN PLACE on the received records (smatrix_apply_packed_dev's kernels),
//   4. answered: the results travel back the same way and k_gather puts them into the caller's op order.
//
// Round 3:
//  * TRANSPORT SEAM.  Everything that talks to the other ranks goes through `Transport`: RCCL (grouped
//    ncclSend/ncclRecv pairs inside one ncclGroupStart/End per exchange, i.e. an alltoallv over xGMI where each peer
//    pair has its own link; bound at run time with dlopen, so a single-GPU user of smatrix.so never needs it), or --
//    SMATRIX_SHARD_TRANSPORT=shm -- a host-staged exchange through a POSIX shared-memory segment.  The second one is a
//    TEST transport: RCCL refuses two ranks on one device, shared memory does not, so the N > 1 branches of this file
//    run with 2 and 8 PROCESSES on one GPU in `pytest -m gpu`.
//  * SPLIT PHASES.  route / apply_routed / finish / wait: all communication of a shard is issued by ONE thread of the
//    library (the comm thread), in the order the calls were made, on its own stream; the host waits of an exchange
//    (partition counts, peer counts) happen THERE, under the host-driven rounds of the op kernels that the caller's
//    thread is running for the previous batch.  The blocking calls are the four phases back to back.
//  * PLACEMENT in the library: the first write batch of an empty matrix is the sample from which hot rows are placed
//    one by one and the tail gets hash ranges of unequal width (plan_placement); stored next to the shard file
//    (<file>.placement) and taken over at reopen.
//  * rowlen / getrow of arbitrary rows, routed to their owners.
#include <dlfcn.h>
#include <sys/mman.h>
#include <rccl/rccl.h>

#include <functional>
#include <mutex>

namespace {

struct Rccl {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*GetVersion)(int*) = nullptr;           // (optional)
  char path[512] = {0};                                 // where the library in use was mapped from
  int version = 0;
  // The copy the process ALREADY holds comes first (RTLD_NOLOAD, by soname and by the path /proc/self/maps shows): a torch
  // process has torch's own librccl mapped, on torch's HIP runtime -- a second copy from /opt/rocm would be a second RCCL on a
  // second runtime in one process (VERDICT r4 #7a).  Only a process that holds none gets one loaded: SMATRIX_RCCL_LIB, then
  // librccl.so.1 / librccl.so by the loader's search path.
  // (ADVICE r5) a handle counts only if it has ncclGetUniqueId -- plugins such as librccl-net.so match "librccl" too and
  // RTLD_NOLOAD succeeds on them; the maps scan compares the file's BASE name with librccl.so[.N...]; the probes for a copy
  // that is already mapped do not pass RTLD_GLOBAL (they would promote torch's private copy into the global scope); load()
  // runs once however many threads ask (std::call_once).
  static bool is_rccl_name(const char* path) {
    const char* b = strrchr(path, '/');
    b = b ? b + 1 : path;
    if (strncmp(b, "librccl.so", 10) != 0) return false;
    for (b += 10; *b; b++)
      if (*b != '.' && (*b < '0' || *b > '9')) return false;
    return true;
  }
  static void* probe(const char* name, int flags) {
    void* h = dlopen(name, flags);
    if (h && !dlsym(h, "ncclGetUniqueId")) { dlclose(h); h = nullptr; }
    return h;
  }
  std::once_flag once;
  bool ok = false;
  bool load() {
    std::call_once(once, [this] { ok = load_once(); });
    return ok;
  }
  bool load_once() {
    const char* names[] = {getenv("SMATRIX_RCCL_LIB"), "librccl.so.1", "librccl.so"};
    for (const char* n : names) {
      if (!n || !*n) continue;
      lib = probe(n, RTLD_NOW | RTLD_NOLOAD);
      if (lib) break;
    }
    if (!lib) {
      if (FILE* f = fopen("/proc/self/maps", "r")) {
        char line[1024];
        while (!lib && fgets(line, sizeof line, f)) {
          char* p = strchr(line, '/');
          if (!p) continue;
          p[strcspn(p, "\n")] = 0;
          if (!is_rccl_name(p)) continue;
          lib = probe(p, RTLD_NOW | RTLD_NOLOAD);
        }
        fclose(f);
      }
    }
    for (const char* n : names) {
      if (lib) break;
      if (!n || !*n) continue;
      lib = probe(n, RTLD_NOW | RTLD_GLOBAL);
    }
    if (!lib) { fprintf(stderr, "libsmatrix: cannot load RCCL: %s\n", dlerror()); return false; }
#define B(field, sym) *(void**)(&field) = dlsym(lib, sym); if (!field) { fprintf(stderr, "libsmatrix: RCCL lacks %s\n", sym); lib = nullptr; return false; }
    B(GetUniqueId, "ncclGetUniqueId") B(CommInitRank, "ncclCommInitRank") B(CommDestroy, "ncclCommDestroy")
    B(GroupStart, "ncclGroupStart") B(GroupEnd, "ncclGroupEnd") B(Send, "ncclSend") B(Recv, "ncclRecv")
    B(GetErrorString, "ncclGetErrorString")
#undef B
    *(void**)(&GetVersion) = dlsym(lib, "ncclGetVersion");
    if (GetVersion) (void)GetVersion(&version);
    Dl_info di;
    if (dladdr(reinterpret_cast<void*>(GetUniqueId), &di) && di.dli_fname) snprintf(path, sizeof path, "%s", di.dli_fname);
    return true;
  }
};
Rccl g_rccl;

#define NCCL_OK(expr)                                                                          \
  do {                                                                                         \
    ncclResult_t r_ = (expr);                                                                  \
    if (r_ != ncclSuccess) {                                                                   \
      char b_[512];                                                                            \
      snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #expr, g_rccl.GetErrorString(r_), __FILE__, __LINE__); \
      smx_die(b_);                                                                             \
    }                                                                                          \
  } while (0)

// ---- the seam ---------------------------------------------------------------------------------------------------
constexpr size_t AG_BYTES = 8192;               // largest contribution to a host allgather (the placement sample)

struct Transport {
  int rank = 0, nranks = 1;
  virtual ~Transport() {}
  virtual const char* name() const = 0;
  // every rank contributes `bytes` (<= AG_BYTES) host bytes; all[] receives nranks * bytes, in rank order
  virtual void allgather_host(const void* mine, void* all, size_t bytes, hipStream_t s) = 0;
  // device alltoallv: send[p] elements of `width` 32-bit words go to peer p, recv[p] come from it; both buffers are
  // contiguous in rank order.  Enqueued on s (the shm transport also waits for s).
  virtual void alltoallv(const uint32_t* d_send, const uint64_t* send, uint32_t* d_recv, const uint64_t* recv, uint32_t width,
                         hipStream_t s) = 0;
};

// one rank, no peer: the exchanges are device copies
struct SelfTransport : Transport {
  const char* name() const override { return "self"; }
  void allgather_host(const void* mine, void* all, size_t bytes, hipStream_t) override { memcpy(all, mine, bytes); }
  void alltoallv(const uint32_t* d_send, const uint64_t* send, uint32_t* d_recv, const uint64_t*, uint32_t width, hipStream_t s) override {
    if (send[0]) HIP_OK(hipMemcpyAsync(d_recv, d_send, send[0] * width * 4, hipMemcpyDeviceToDevice, s));
  }
};

struct RcclTransport : Transport {
  ncclComm_t comm = nullptr;
  bool self_over_rccl = false;                  // SMATRIX_SHARD_FORCE_RCCL=1: the rank's own share travels through RCCL too
  uint8_t* d_ag = nullptr;                      // [nranks + 1][AG_BYTES]: slot nranks = what this rank sends
  uint8_t* h_ag = nullptr;                      // pinned mirror
  const char* name() const override { return "rccl"; }
  std::string failed;                           // why the communicator could not be created (smatrix_shard_open then returns NULL)
  RcclTransport(int r, int n, const void* id128, bool self_too) {
    rank = r; nranks = n; self_over_rccl = self_too;
    ncclUniqueId id;
    ncclResult_t rc = ncclSuccess;
    if (id128) memcpy(&id, id128, sizeof id);
    else rc = g_rccl.GetUniqueId(&id);          // (one rank, forced: nobody to agree with)
    // a refused communicator is the CALLER's to handle (open returns NULL like any failed open, src/smatrix.c:77-78,:92-96):
    // the first RCCL contact of a process is where a missing library, a bad id or a mis-set environment shows
    if (rc == ncclSuccess) rc = g_rccl.CommInitRank(&comm, nranks, id, rank);
    if (rc != ncclSuccess) { failed = std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(rc); comm = nullptr; return; }
    dev_malloc(&d_ag, (size_t)(nranks + 1) * AG_BYTES);
    HIP_OK(hipHostMalloc(&h_ag, (size_t)(nranks + 1) * AG_BYTES));
  }
  ~RcclTransport() override {
    if (comm) (void)g_rccl.CommDestroy(comm);
    if (d_ag) (void)hipFree(d_ag);
    if (h_ag) (void)hipHostFree(h_ag);
  }
  void allgather_host(const void* mine, void* all, size_t bytes, hipStream_t s) override {
    if (bytes > AG_BYTES) smx_die("internal: allgather_host contribution too large");
    memcpy(h_ag + (size_t)nranks * AG_BYTES, mine, bytes);
    HIP_OK(hipMemcpyAsync(d_ag + (size_t)nranks * AG_BYTES, h_ag + (size_t)nranks * AG_BYTES, bytes, hipMemcpyHostToDevice, s));
    NCCL_OK(g_rccl.GroupStart());
    for (int p = 0; p < nranks; p++) {
      if (p == rank && !self_over_rccl) continue;
      NCCL_OK(g_rccl.Send(d_ag + (size_t)nranks * AG_BYTES, bytes, ncclUint8, p, comm, s));
      NCCL_OK(g_rccl.Recv(d_ag + (size_t)p * AG_BYTES, bytes, ncclUint8, p, comm, s));
    }
    NCCL_OK(g_rccl.GroupEnd());
    HIP_OK(hipMemcpyAsync(h_ag, d_ag, (size_t)nranks * AG_BYTES, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    for (int p = 0; p < nranks; p++)
      memcpy(static_cast<uint8_t*>(all) + (size_t)p * bytes, p == rank && !self_over_rccl ? static_cast<const uint8_t*>(mine) : h_ag + (size_t)p * AG_BYTES, bytes);
  }
  void alltoallv(const uint32_t* d_send, const uint64_t* send, uint32_t* d_recv, const uint64_t* recv, uint32_t width, hipStream_t s) override {
    uint64_t so = 0, ro = 0;
    NCCL_OK(g_rccl.GroupStart());
    for (int p = 0; p < nranks; p++) {
      if (p == rank && !self_over_rccl) {
        if (send[p]) HIP_OK(hipMemcpyAsync(d_recv + ro * width, d_send + so * width, send[p] * width * 4, hipMemcpyDeviceToDevice, s));
      } else {
        if (send[p]) NCCL_OK(g_rccl.Send(d_send + so * width, send[p] * width, ncclUint32, p, comm, s));
        if (recv[p]) NCCL_OK(g_rccl.Recv(d_recv + ro * width, recv[p] * width, ncclUint32, p, comm, s));
      }
      so += send[p];
      ro += recv[p];
    }
    NCCL_OK(g_rccl.GroupEnd());
  }
};

// Host-staged exchange through one POSIX shared-memory object (the 128-byte id holds its name).  Layout: a header with
// a counter barrier, one AG_BYTES area per rank, then nranks x nranks mailboxes of `slot` bytes (from -> to).  Messages
// larger than a mailbox travel in rounds.  A TEST transport: it exists so that more than one rank can share a GPU.
struct ShmTransport : Transport {
  struct Header {
    std::atomic<uint32_t> arrived, generation;
    std::atomic<uint32_t> attached;
    uint32_t pad;
  };
  std::string shm_name;
  uint8_t* base = nullptr;
  size_t total = 0, slot = 0;
  Header* hdr = nullptr;
  const char* name() const override { return "shm"; }
  uint8_t* ag_area(int r) { return base + 4096 + (size_t)r * AG_BYTES; }
  uint8_t* box(int from, int to) { return base + 4096 + (size_t)nranks * AG_BYTES + ((size_t)from * nranks + to) * slot; }
  ShmTransport(int r, int n, const void* id128) {
    rank = r; nranks = n;
    char nm[SMATRIX_SHARD_ID_BYTES + 1];
    memcpy(nm, id128, SMATRIX_SHARD_ID_BYTES);
    nm[SMATRIX_SHARD_ID_BYTES] = 0;
    if (nm[0] != '/') smx_die("shm shard transport: the id must be a shared-memory object name (\"/name\")");
    shm_name = nm;
    size_t mb = 256;
    if (const char* e = getenv("SMATRIX_SHARD_SHM_MB")) mb = std::max<size_t>(8, strtoull(e, nullptr, 10));
    slot = ((mb << 20) / ((size_t)n * n)) & ~(size_t)4095;
    if (slot < 65536) slot = 65536;
    total = 4096 + (size_t)n * AG_BYTES + (size_t)n * n * slot;
    const int fd = shm_open(nm, O_RDWR | O_CREAT, 0600);
    if (fd < 0) smx_die("shm shard transport: shm_open failed");
    if (ftruncate(fd, (off_t)total) != 0) smx_die("shm shard transport: ftruncate failed");   // (same size on every rank; new pages read zero)
    void* p = mmap(nullptr, total, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (p == MAP_FAILED) smx_die("shm shard transport: mmap failed");
    base = static_cast<uint8_t*>(p);
    hdr = reinterpret_cast<Header*>(base);
    hdr->attached.fetch_add(1);
    barrier();                                   // everybody is attached
  }
  ~ShmTransport() override {
    if (!base) return;
    barrier();
    if (rank == 0) shm_unlink(shm_name.c_str());
    munmap(base, total);
  }
  void barrier() {
    const uint32_t gen = hdr->generation.load(std::memory_order_acquire);
    if (hdr->arrived.fetch_add(1, std::memory_order_acq_rel) + 1 == (uint32_t)nranks) {
      hdr->arrived.store(0, std::memory_order_relaxed);
      hdr->generation.fetch_add(1, std::memory_order_acq_rel);
      return;
    }
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t spins = 0;
    while (hdr->generation.load(std::memory_order_acquire) == gen) {
      if (++spins > 2000) { usleep(50); }
      if ((spins & 0xfff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(300))
        smx_die("shm shard transport: a peer did not arrive (collective calls out of step, or a rank died)");
    }
  }
  void allgather_host(const void* mine, void* all, size_t bytes, hipStream_t) override {
    if (bytes > AG_BYTES) smx_die("internal: allgather_host contribution too large");
    memcpy(ag_area(rank), mine, bytes);
    barrier();
    for (int p = 0; p < nranks; p++) memcpy(static_cast<uint8_t*>(all) + (size_t)p * bytes, ag_area(p), bytes);
    barrier();
  }
  void alltoallv(const uint32_t* d_send, const uint64_t* send, uint32_t* d_recv, const uint64_t* recv, uint32_t width, hipStream_t s) override {
    HIP_OK(hipStreamSynchronize(s));             // what is sent was produced on s
    uint64_t mx = 0;
    for (int p = 0; p < nranks; p++) mx = std::max<uint64_t>(mx, std::max(send[p], recv[p]) * width * 4);
    std::vector<uint64_t> all(nranks);
    allgather_host(&mx, all.data(), 8, s);
    for (uint64_t v : all) mx = std::max(mx, v);
    const uint64_t rounds = (mx + slot - 1) / slot;
    for (uint64_t k = 0; k < rounds; k++) {
      uint64_t so = 0, ro = 0;
      for (int p = 0; p < nranks; p++) {
        const uint64_t bytes = send[p] * width * 4, lo = std::min<uint64_t>(bytes, k * slot), hi = std::min<uint64_t>(bytes, (k + 1) * slot);
        if (hi > lo) HIP_OK(hipMemcpy(box(rank, p), reinterpret_cast<const uint8_t*>(d_send + so * width) + lo, hi - lo, hipMemcpyDeviceToHost));
        so += send[p];
      }
      barrier();
      for (int p = 0; p < nranks; p++) {
        const uint64_t bytes = recv[p] * width * 4, lo = std::min<uint64_t>(bytes, k * slot), hi = std::min<uint64_t>(bytes, (k + 1) * slot);
        if (hi > lo) HIP_OK(hipMemcpy(reinterpret_cast<uint8_t*>(d_recv + ro * width) + lo, box(p, rank), hi - lo, hipMemcpyHostToDevice));
        ro += recv[p];
      }
      barrier();
    }
  }
};

bool transport_is_shm() {
  const char* t = getenv("SMATRIX_SHARD_TRANSPORT");
  return t && !strcmp(t, "shm");
}

// ---- placement: planning (host) and its file ------------------------------------------------------------------------
struct PlacementPlan {
  int world = 1;
  bool have_cuts = false;
  std::vector<uint32_t> cuts;                        // world - 1 ascending cut points
  std::vector<std::pair<uint32_t, uint32_t>> place;   // {x, owner}, sorted by x
};

// Skew-aware placement (SURVEY.md 8e "skew handling"; the same algorithm as libsmatrix_amd/sharded.py plan_placement).
// counts: ops seen per row id in a sample of `total` ops.  The `top` hottest rows are assigned one by one, longest
// processing time first, to the least loaded shard; the flat tail gets hash ranges of UNEQUAL width that fill every shard
// to the same level.  Deterministic: every rank computes the same plan from the same gathered counts.
PlacementPlan plan_placement(std::vector<std::pair<uint32_t, uint64_t>> counts, uint64_t total, int world, size_t top) {
  std::sort(counts.begin(), counts.end(), [](const std::pair<uint32_t, uint64_t>& a, const std::pair<uint32_t, uint64_t>& b) {
    return a.second != b.second ? a.second > b.second : a.first < b.first;
  });
  if (counts.size() > top) counts.resize(top);
  std::vector<double> load(world, 0.0);
  PlacementPlan pl;
  pl.world = world;
  uint64_t hot_ops = 0;
  for (const auto& c : counts) {
    int r = 0;
    for (int i = 1; i < world; i++) if (load[i] < load[r]) r = i;
    load[r] += (double)c.second;
    pl.place.push_back({c.first, (uint32_t)r});
    hot_ops += c.second;
  }
  std::sort(pl.place.begin(), pl.place.end());
  const double tail = total > hot_ops ? (double)(total - hot_ops) : 0.0;
  std::vector<double> order(load);
  std::sort(order.begin(), order.end());
  double level = order.back() + tail;
  for (int k = 1; k <= world; k++) {                 // the k least loaded shards share the tail
    double acc = 0;
    for (int i = 0; i < k; i++) acc += order[i];
    level = (tail + acc) / k;
    if (k == world || level <= order[k]) break;
  }
  double tot_w = 0;
  std::vector<double> width(world);
  for (int r = 0; r < world; r++) { width[r] = std::max(level - load[r], 0.0); tot_w += width[r]; }
  if (tot_w <= 0) tot_w = 1.0;
  double run = 0;
  for (int r = 0; r + 1 < world; r++) {
    run += width[r] / tot_w;
    const double c = run * 4294967296.0;
    pl.cuts.push_back(c >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)c);
  }
  pl.have_cuts = world > 1;
  return pl;
}

// <file>.placement: the JSON libsmatrix_amd/sharded.py writes -- {"world": W, "cuts": [..] | null, "place": [[x, owner], ..]}
std::string placement_to_json(const PlacementPlan& pl) {
  std::string s = "{\"world\": " + std::to_string(pl.world) + ", \"cuts\": ";
  if (!pl.have_cuts) s += "null";
  else {
    s += "[";
    for (size_t i = 0; i < pl.cuts.size(); i++) s += (i ? ", " : "") + std::to_string(pl.cuts[i]);
    s += "]";
  }
  s += ", \"place\": [";
  for (size_t i = 0; i < pl.place.size(); i++)
    s += (i ? ", [" : "[") + std::to_string(pl.place[i].first) + ", " + std::to_string(pl.place[i].second) + "]";
  s += "]}";
  return s;
}

bool placement_from_json(const std::string& t, PlacementPlan* pl) {
  auto number_after = [&](size_t at, uint64_t* v) -> size_t {   // the next run of digits at/after `at`
    while (at < t.size() && !isdigit((unsigned char)t[at])) at++;
    if (at >= t.size()) return std::string::npos;
    uint64_t x = 0;
    while (at < t.size() && isdigit((unsigned char)t[at])) x = x * 10 + (uint64_t)(t[at++] - '0');
    *v = x;
    return at;
  };
  const size_t w = t.find("\"world\""), c = t.find("\"cuts\""), p = t.find("\"place\"");
  if (w == std::string::npos || c == std::string::npos || p == std::string::npos) return false;
  uint64_t v = 0;
  if (number_after(w + 7, &v) == std::string::npos || v < 1 || v > MAX_SHARDS) return false;
  pl->world = (int)v;
  pl->cuts.clear(); pl->place.clear();
  size_t at = t.find_first_not_of(" :", c + 6);
  pl->have_cuts = at != std::string::npos && t[at] == '[';
  if (pl->have_cuts) {
    const size_t end = t.find(']', at);
    if (end == std::string::npos) return false;
    for (size_t q = at; (q = number_after(q, &v)) != std::string::npos && q <= end;) pl->cuts.push_back((uint32_t)v);
    if ((int)pl->cuts.size() != pl->world - 1) return false;
  }
  at = t.find('[', p + 7);
  if (at == std::string::npos) return false;
  const size_t end = t.rfind(']');
  for (size_t q = at + 1; q < end;) {
    uint64_t x = 0, o = 0;
    q = number_after(q, &x);
    if (q == std::string::npos || q >= end) break;
    q = number_after(q, &o);
    if (q == std::string::npos) return false;
    if (o >= (uint64_t)pl->world) return false;
    pl->place.push_back({(uint32_t)x, (uint32_t)o});
  }
  return true;
}

// ---- a routed batch ----------------------------------------------------------------------------------------------------
struct Routed {
  int op = 0;
  size_t n = 0;
  uint32_t width = 2;
  uint64_t total = 0;                                   // records this rank received = ops its shard applies
  uint64_t send[MAX_SHARDS], recv[MAX_SHARDS];
  const uint32_t *d_x = nullptr, *d_y = nullptr, *d_v = nullptr;
  bool inputs_ready = false, then_get = false, in_use = false, in_place = false;
  DevBuf<uint32_t> perm, packed, recvbuf, res, res2, back, back2;
  hipEvent_t ev_in = nullptr, ev_routed = nullptr, ev_applied = nullptr, ev_done = nullptr;
  uint32_t *d_out = nullptr, *d_out2 = nullptr;
  uint64_t task_route = 0;                              // ticket of the comm-thread task that routes it
};

}  // namespace

struct smatrix_routed { Routed r; };

struct smatrix_shard {
  smatrix_t* local = nullptr;
  int rank = 0, nranks = 1, device = 0;
  Transport* tr = nullptr;
  // placement: device copies of the cut points and the hot-row table
  uint32_t* d_cuts = nullptr;
  uint32_t* d_place = nullptr;
  uint32_t place_slots = 0;
  PlacementPlan plan;                                   // what they were built from (equal ranges: no cuts, no rows)
  bool placed = false;                                  // settled (stored, planned, or decided to stay with equal ranges)
  bool place_dirty = false;                             // to be written next to the shard file at close
  std::mutex pool_mu;                                   // the routed pool's in_use flags (routed_take / shard_wait)
  bool place_saved = false;                             // ... and has been (shard_persist_placement)
  bool auto_place = true;                               // SMATRIX_SHARD_PLACE=0: equal hash ranges
  std::string fname;
  unsigned long long* d_work = nullptr;                 // 2 x 64 counters of the partition kernels
  uint64_t* h_cnt = nullptr;                            // pinned: partition counts
  uint64_t ops_applied = 0, calls = 0;
  // the comm thread: every exchange of this shard, in call order, on `cs`
  hipStream_t cs = nullptr;
  std::thread comm;
  std::mutex qmu;
  std::condition_variable qcv;
  std::deque<std::pair<uint64_t, std::function<void()>>> queue;
  uint64_t issued = 0, done = 0;
  bool stop = false;
  smatrix_routed pool[4];
  DevBuf<uint32_t> t_x, t_y, t_a, t_b, t_c;             // scratch of the rowlen / getrow routes
  DevBuf<uint64_t> t_off, t_off2, t_pairs, t_pairs2;
  std::mutex mu;                                        // the blocking entry points, one at a time
};

namespace {

void comm_main(smatrix_shard* sh) {
  HIP_OK(hipSetDevice(sh->device));
  std::unique_lock<std::mutex> l(sh->qmu);
  for (;;) {
    sh->qcv.wait(l, [&] { return sh->stop || !sh->queue.empty(); });
    if (sh->queue.empty()) return;
    auto task = std::move(sh->queue.front());
    sh->queue.pop_front();
    l.unlock();
    task.second();
    l.lock();
    sh->done = task.first;
    sh->qcv.notify_all();
  }
}
uint64_t comm_submit(smatrix_shard* sh, std::function<void()> f) {
  std::lock_guard<std::mutex> l(sh->qmu);
  const uint64_t ticket = ++sh->issued;
  sh->queue.push_back({ticket, std::move(f)});
  sh->qcv.notify_all();
  return ticket;
}
void comm_wait(smatrix_shard* sh, uint64_t ticket) {
  std::unique_lock<std::mutex> l(sh->qmu);
  sh->qcv.wait(l, [&] { return sh->done >= ticket; });
}

void shard_upload_placement(smatrix_shard* sh) {
  HIP_OK(hipSetDevice(sh->device));
  if (sh->d_cuts) { (void)hipFree(sh->d_cuts); sh->d_cuts = nullptr; }
  if (sh->d_place) { (void)hipFree(sh->d_place); sh->d_place = nullptr; }
  sh->place_slots = 0;
  const PlacementPlan& pl = sh->plan;
  if (pl.have_cuts && sh->nranks > 1) {
    dev_malloc(&sh->d_cuts, (size_t)(sh->nranks - 1) * 4);
    HIP_OK(hipMemcpy(sh->d_cuts, pl.cuts.data(), (size_t)(sh->nranks - 1) * 4, hipMemcpyHostToDevice));
  }
  if (!pl.place.empty()) {
    uint32_t slots = 16;
    while (slots < 2 * pl.place.size()) slots *= 2;
    if (slots > PLACE_MAX_SLOTS) smx_die("shard placement: too many rows placed one by one");
    std::vector<uint32_t> tab((size_t)slots * 2, 0u);
    for (const auto& e : pl.place) {
      uint32_t i = smx_fmix32(e.first) & (slots - 1u);
      while (tab[2 * i + 1]) i = (i + 1) & (slots - 1u);
      tab[2 * i] = e.first;
      tab[2 * i + 1] = e.second + 1u;
    }
    dev_malloc(&sh->d_place, (size_t)slots * 8);
    HIP_OK(hipMemcpy(sh->d_place, tab.data(), (size_t)slots * 8, hipMemcpyHostToDevice));
    sh->place_slots = slots;
  }
}

// The placement goes next to the shard file WHEN IT IS DECIDED (ADVICE r3): rows never move, so a reopen must route the same
// way -- and with the background flusher rows reach the shard file long before close.  A process that died before
// smatrix_shard_close used to leave shard files with hot rows placed one by one and no .placement beside them, which the
// reopen then refused.  tmp + fsync + rename (+ fsync of the directory entry is left to the file system): the file is
// either the old one or the complete new one.  Close writes it once more (a refresh).
void shard_persist_placement(smatrix_shard* sh) {
  if (sh->fname.empty() || !(sh->plan.have_cuts || !sh->plan.place.empty())) return;
  const std::string pf = sh->fname + ".placement", tmp = pf + ".tmp";
  FILE* f = fopen(tmp.c_str(), "w");
  if (!f) { perror("cannot write the shard placement"); smx_die("shard placement: cannot create the .placement file"); }
  const std::string t = placement_to_json(sh->plan);
  const bool ok = fwrite(t.data(), 1, t.size(), f) == t.size() && fflush(f) == 0 && fsync(fileno(f)) == 0;
  if (fclose(f) != 0 || !ok) smx_die("shard placement: short write of the .placement file");
  if (rename(tmp.c_str(), pf.c_str()) != 0) { perror("rename"); smx_die("shard placement: cannot move the .placement file into place"); }
  sh->place_dirty = false;
  sh->place_saved = true;
}

// COLLECTIVE, on the comm thread, before the first batch is partitioned: which shard owns which row?
//   * a placement stored next to the shard files (read at open) -> that one, if all ranks hold the same;
//   * an EMPTY matrix and a write batch -> planned from a sample of this batch (plan_placement);
//   * rows but no stored placement (files written under equal ranges) -> equal ranges plus the rows found away from
//     their range (a handful); many such rows mean the .placement file of a planned matrix is missing: refuse.
void shard_settle_placement(smatrix_shard* sh, const Routed& r, bool write) {
  if (sh->placed) return;
  const int R = sh->nranks;
  hipStream_t s = sh->cs;
  smatrix_stats_t st;
  smatrix_stats(sh->local, &st);
  struct Info { uint64_t rows, have_stored, hash, n; } mine = {st.rows, 0, 0, (uint64_t)r.n};
  std::string stored;
  if (sh->place_dirty == false && (sh->plan.have_cuts || !sh->plan.place.empty())) {   // loaded at open or set by the caller
    stored = placement_to_json(sh->plan);
    mine.have_stored = 1;
    for (unsigned char c : stored) mine.hash = (mine.hash ^ c) * 0x100000001b3ULL;
  }
  std::vector<Info> all(R);
  sh->tr->allgather_host(&mine, all.data(), sizeof mine, s);
  uint64_t rows = 0, n_stored = 0;
  for (const Info& i : all) { rows += i.rows; n_stored += i.have_stored; }
  if (n_stored) {
    for (const Info& i : all)
      if (!i.have_stored || i.hash != mine.hash) smx_die("shard placement: the ranks' stored placements differ (or some shard files lack their .placement)");
    sh->placed = true;                                   // already uploaded when it was loaded / set
    return;
  }
  if (rows == 0 && !write) return;                       // reads of an empty matrix find nothing wherever they go: decide later
  sh->placed = true;
  if (rows) {
    // rows exist, nothing stored: they must sit where equal ranges put them
    std::vector<uint32_t> disp(600);
    const size_t nd = smatrix_displaced_rows(sh->local, (uint32_t)sh->rank, (uint32_t)R, disp.data(), disp.size());
    uint64_t cnt = nd;
    std::vector<uint64_t> cnts(R);
    sh->tr->allgather_host(&cnt, cnts.data(), 8, s);
    uint64_t tot = 0;
    for (uint64_t c : cnts) tot += c;
    if (tot > 512)
      smx_die("shard placement: rows live away from their equal-range owner and no stored placement was found -- shard "
              "files written under a planned placement need their .placement file");
    if (tot) {
      // (a handful of rows placed by an earlier, smaller plan: keep them where they are)
      struct Pack { uint32_t n, x[600]; } pk;
      static_assert(sizeof(Pack) <= AG_BYTES, "fits one allgather");
      pk.n = (uint32_t)std::min<size_t>(nd, 600);
      memcpy(pk.x, disp.data(), pk.n * 4);
      std::vector<Pack> every(R);
      sh->tr->allgather_host(&pk, every.data(), sizeof pk, s);
      sh->plan = PlacementPlan();
      sh->plan.world = R;
      for (int p = 0; p < R; p++)
        for (uint32_t k = 0; k < every[p].n; k++) sh->plan.place.push_back({every[p].x[k], (uint32_t)p});
      std::sort(sh->plan.place.begin(), sh->plan.place.end());
      shard_upload_placement(sh);
      shard_persist_placement(sh);
    }
    return;
  }
  if (!sh->auto_place || R == 1) return;                 // equal hash ranges
  // the sample: the first 2^20 ops of this rank's batch, counted on the host; its TOP most frequent row ids travel
  constexpr size_t TOP = 256, SAMPLE = (size_t)1 << 20;
  struct Share { uint64_t n; uint32_t k, pad; uint32_t x[TOP]; uint32_t c[TOP]; } sm;
  static_assert(sizeof(Share) <= AG_BYTES, "fits one allgather");
  memset(&sm, 0, sizeof sm);
  const size_t ns = std::min(r.n, SAMPLE);
  sm.n = ns;
  if (ns) {
    std::vector<uint32_t> xs(ns);
    if (!r.inputs_ready) HIP_OK(hipStreamWaitEvent(s, r.ev_in, 0));
    HIP_OK(hipMemcpyAsync(xs.data(), r.d_x, ns * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    std::sort(xs.begin(), xs.end());
    std::vector<std::pair<uint32_t, uint32_t>> runs;    // {count, x}
    for (size_t i = 0; i < ns;) {
      size_t j = i;
      while (j < ns && xs[j] == xs[i]) j++;
      runs.push_back({(uint32_t)(j - i), xs[i]});
      i = j;
    }
    const size_t k = std::min(runs.size(), TOP);
    std::partial_sort(runs.begin(), runs.begin() + k, runs.end(), [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) {
      return a.first != b.first ? a.first > b.first : a.second < b.second;
    });
    sm.k = (uint32_t)k;
    for (size_t i = 0; i < k; i++) { sm.x[i] = runs[i].second; sm.c[i] = runs[i].first; }
  }
  std::vector<Share> shares(R);
  sh->tr->allgather_host(&sm, shares.data(), sizeof sm, s);
  std::map<uint32_t, uint64_t> merged;
  uint64_t total = 0;
  for (const Share& q : shares) {
    total += q.n;
    for (uint32_t i = 0; i < q.k; i++) merged[q.x[i]] += q.c[i];
  }
  sh->plan = plan_placement(std::vector<std::pair<uint32_t, uint64_t>>(merged.begin(), merged.end()), total, R, TOP);
  sh->place_dirty = true;
  shard_upload_placement(sh);
  shard_persist_placement(sh);                           // on disk before the first op of this batch is applied anywhere
}

// the routing of one batch, on the comm thread: placement (first time), partition, counts, records
void shard_route_task(smatrix_shard* sh, Routed* r) {
  hipStream_t s = sh->cs;
  const int R = sh->nranks;
  sh->calls++;
  shard_settle_placement(sh, *r, r->op != OP_GET);
  if (!r->inputs_ready) HIP_OK(hipStreamWaitEvent(s, r->ev_in, 0));
  r->perm.need(std::max<size_t>(r->n, 1));
  r->packed.need(std::max<size_t>(r->n, 1) * r->width);
  if (smatrix_partition_packed_dev(r->n, r->d_x, r->d_y, r->d_v, (uint32_t)R, r->send, sh->d_work, r->perm.p, r->packed.p, sh->d_place,
                                   sh->place_slots, sh->d_cuts, s) != 0)
    smx_die("shard: partition failed");                  // (synchronises s once: counts on the host)
  // counts: every rank's row of the R x R matrix
  std::vector<uint64_t> all((size_t)R * R);
  sh->tr->allgather_host(r->send, all.data(), (size_t)R * 8, s);
  r->total = 0;
  for (int p = 0; p < R; p++) { r->recv[p] = all[(size_t)p * R + sh->rank]; r->total += r->recv[p]; }
  if (r->total >= (1ull << 32)) smx_die("sharded batch too large for one shard (>= 2^32 ops routed to one rank)");
  r->res.need(std::max<uint64_t>(r->total, 1));
  r->res2.need(std::max<uint64_t>(r->total, 1));
  // one rank: everything is this rank's own share -- the partitioned records are applied where they are and the results
  // gathered from where the kernels wrote them (no device copies standing in for an exchange)
  r->in_place = R == 1 && !strcmp(sh->tr->name(), "self");
  if (!r->in_place) {
    r->recvbuf.need(std::max<uint64_t>(r->total, 1) * r->width);
    sh->tr->alltoallv(r->packed.p, r->send, r->recvbuf.p, r->recv, r->width, s);
  }
  HIP_OK(hipEventRecord(r->ev_routed, s));
}

// results back and into the caller's order, on the comm thread
void shard_finish_task(smatrix_shard* sh, Routed* r) {
  hipStream_t s = sh->cs;
  HIP_OK(hipStreamWaitEvent(s, r->ev_applied, 0));
  const uint32_t *b1 = r->res.p, *b2 = r->res2.p;          // (one rank, in place: the results are gathered from where they are)
  if (!r->in_place) {
    r->back.need(std::max<size_t>(r->n, 1));
    sh->tr->alltoallv(r->res.p, r->recv, r->back.p, r->send, 1, s);
    b1 = r->back.p;
    if (r->then_get) {
      r->back2.need(std::max<size_t>(r->n, 1));
      sh->tr->alltoallv(r->res2.p, r->recv, r->back2.p, r->send, 1, s);
      b2 = r->back2.p;
    }
  }
  if (r->n && r->then_get && r->d_out && r->d_out2) {       // both result sets in one pass over the permutation
    hipLaunchKernelGGL(k_gather2, dim3(blocks_for(r->n)), dim3(256), 0, s, (uint32_t)r->n, b1, b2, r->perm.p, r->d_out, r->d_out2);
    HIP_OK(hipGetLastError());
  } else {
    if (r->n && r->d_out) smatrix_gather_dev(r->n, b1, r->perm.p, r->d_out, s);
    if (r->n && r->then_get && r->d_out2) smatrix_gather_dev(r->n, b2, r->perm.p, r->d_out2, s);
  }
  HIP_OK(hipEventRecord(r->ev_done, s));
}

smatrix_routed* routed_take(smatrix_shard* sh) {
  // (the pool is shared by the blocking calls, which hold sh->mu, and the split-phase calls, which do not: its flags have
  //  their own small lock -- ADVICE r3)
  std::lock_guard<std::mutex> pg(sh->pool_mu);
  for (smatrix_routed& h : sh->pool)
    if (!h.r.in_use) {
      Routed& r = h.r;
      r.in_use = true;
      if (!r.ev_in) {
        HIP_OK(hipEventCreateWithFlags(&r.ev_in, hipEventDisableTiming));
        HIP_OK(hipEventCreateWithFlags(&r.ev_routed, hipEventDisableTiming));
        HIP_OK(hipEventCreateWithFlags(&r.ev_applied, hipEventDisableTiming));
        HIP_OK(hipEventCreateWithFlags(&r.ev_done, hipEventDisableTiming));
      }
      return &h;
    }
  smx_die("shard: more than 4 routed batches in flight (smatrix_shard_wait releases them)");
}

// arguments that can differ per rank are checked BEFORE any collective, and a violation is fatal: a rank that returned an
// error code here would leave its peers waiting in the exchange (ADVICE r2)
void shard_check_args(int op, size_t n, const uint32_t* d_x, const uint32_t* d_y, const uint32_t* d_v) {
  if (op < OP_GET || op > OP_DECR) smx_die("shard: bad op code");
  if (n >= (1ull << 32)) smx_die("shard: batch too large (n must be < 2^32)");
  if (n && (!d_x || !d_y)) smx_die("shard: NULL op arrays");
  if (n && op != OP_GET && !d_v) smx_die("shard: a write batch needs values");
}

smatrix_routed* shard_route(smatrix_shard* sh, int op, size_t n, const uint32_t* d_x, const uint32_t* d_y, const uint32_t* d_v,
                            bool inputs_ready, hipStream_t user) {
  shard_check_args(op, n, d_x, d_y, d_v);
  HIP_OK(hipSetDevice(sh->device));
  smatrix_routed* h = routed_take(sh);
  Routed& r = h->r;
  r.op = op; r.n = n; r.d_x = d_x; r.d_y = d_y; r.d_v = op == OP_GET ? nullptr : d_v;
  r.width = r.d_v ? 3u : 2u;
  r.inputs_ready = inputs_ready;
  r.then_get = false;
  r.d_out = r.d_out2 = nullptr;
  if (!inputs_ready) HIP_OK(hipEventRecord(r.ev_in, user));
  r.task_route = comm_submit(sh, [sh, h] { shard_route_task(sh, &h->r); });
  return h;
}

void shard_apply_routed(smatrix_shard* sh, smatrix_routed* h, bool then_get, hipStream_t user) {
  Routed& r = h->r;
  comm_wait(sh, r.task_route);
  if (then_get && r.op == OP_GET) smx_die("shard: apply-then-get needs a write batch");
  HIP_OK(hipSetDevice(sh->device));
  HIP_OK(hipStreamWaitEvent(user, r.ev_routed, 0));
  r.then_get = then_get;
  if (r.total) {
    const uint32_t* rec = r.in_place ? r.packed.p : r.recvbuf.p;
    smatrix_apply_packed_dev(sh->local, r.op, r.total, rec, r.width, r.res.p, user);      // host-driven rounds for writers
    if (then_get) smatrix_apply_packed_dev(sh->local, OP_GET, r.total, rec, r.width, r.res2.p, user);   // reads {x,y} of the same records
  }
  sh->ops_applied += r.total * (then_get ? 2 : 1);
  HIP_OK(hipEventRecord(r.ev_applied, user));
}

void shard_finish(smatrix_shard* sh, smatrix_routed* h, uint32_t* d_out, uint32_t* d_out2) {
  Routed& r = h->r;
  r.d_out = d_out; r.d_out2 = d_out2;
  comm_wait(sh, comm_submit(sh, [sh, h] { shard_finish_task(sh, &h->r); }));
}

void shard_wait(smatrix_shard* sh, smatrix_routed* h, hipStream_t user) {
  HIP_OK(hipSetDevice(sh->device));
  HIP_OK(hipStreamWaitEvent(user, h->r.ev_done, 0));
  std::lock_guard<std::mutex> pg(sh->pool_mu);
  h->r.in_use = false;
}

// op on every rank's n ops; then_get: a get on the same keys right behind it, same exchange
int shard_apply(smatrix_shard* sh, int op, bool then_get, size_t n, const uint32_t* d_x, const uint32_t* d_y, const uint32_t* d_v,
                uint32_t* d_out, uint32_t* d_out2, void* hip_stream) {
  std::lock_guard<std::mutex> g(sh->mu);
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  smatrix_routed* h = shard_route(sh, op, n, d_x, d_y, d_v, false, s);
  shard_apply_routed(sh, h, then_get, s);
  shard_finish(sh, h, d_out, d_out2);
  shard_wait(sh, h, s);
  if (!hip_stream) HIP_OK(hipStreamSynchronize(s));
  return 0;
}

// ---- rowlen / getrow of arbitrary rows: routed to the owners (kernels of this file only) --------------------------------
__global__ __launch_bounds__(256) void k_caps_from_offsets(uint32_t n, const uint64_t* __restrict__ off, uint32_t* __restrict__ caps) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { const uint64_t c = off[i + 1] - off[i]; caps[i] = c > 0xffffffffull ? 0xffffffffu : (uint32_t)c; }
}
// out[i] = sum of in[j * stride] for j < i (n + 1 outputs), one workgroup
__global__ __launch_bounds__(1024) void k_excl_scan_u32(uint32_t n, const uint32_t* __restrict__ in, uint32_t stride, uint64_t* __restrict__ out) {
  __shared__ uint64_t l_w[16];
  __shared__ uint64_t l_run;
  if (threadIdx.x == 0) l_run = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint32_t t0 = 0; t0 < n; t0 += 1024) {
    const uint32_t t = t0 + threadIdx.x;
    const uint64_t v = t < n ? in[(size_t)t * stride] : 0;
    uint64_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t up = ((uint64_t)(uint32_t)__shfl_up((int)(inc >> 32), o) << 32) | (uint32_t)__shfl_up((int)inc, o);
      if (lane >= (uint32_t)o) inc += up;
    }
    if (lane == 63) l_w[w] = inc;
    __syncthreads();
    uint64_t before = l_run;
    for (uint32_t k = 0; k < w; k++) before += l_w[k];
    if (t < n) out[t] = before + inc - v;
    __syncthreads();
    if (threadIdx.x == 1023) l_run = before + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) out[n] = l_run;
}
// caller row i <- partitioned row perm[i]: its count and its pairs (one wave per row)
__global__ __launch_bounds__(256) void k_rows_unpermute(uint32_t n, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ cnt_p,
                                                        const uint64_t* __restrict__ off_p, const uint64_t* __restrict__ pairs_p,
                                                        const uint64_t* __restrict__ off, uint64_t* __restrict__ pairs, uint32_t* __restrict__ counts) {
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63, nwaves = (gridDim.x * blockDim.x) >> 6;
  for (uint32_t i = wave; i < n; i += nwaves) {
    const uint32_t q = perm[i], c = cnt_p[q];
    const uint64_t src = off_p[q], dst = off[i];
    for (uint32_t k = lane; k < c; k += 64) pairs[dst + k] = pairs_p[src + k];
    if (lane == 0) counts[i] = c;
  }
}

// segment sums of the caps that sit in word 1 of width-2 records: sums[p] = sum over records [lo_p, hi_p)
void seg_cap_sums(const uint64_t* off_dev_all, uint32_t n_records, const uint64_t* counts, int R, uint64_t* sums, hipStream_t s) {
  std::vector<uint64_t> bounds(R + 1, 0), vals(R + 1);
  for (int p = 0; p < R; p++) bounds[p + 1] = bounds[p] + counts[p];
  (void)n_records;
  for (int p = 0; p <= R; p++) HIP_OK(hipMemcpyAsync(&vals[p], off_dev_all + bounds[p], 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  for (int p = 0; p < R; p++) sums[p] = vals[p + 1] - vals[p];
}

void shard_rowlen_task(smatrix_shard* sh, size_t n, const uint32_t* d_x, uint32_t* d_out, hipEvent_t ev_in, hipEvent_t ev_done) {
  hipStream_t s = sh->cs;
  const int R = sh->nranks;
  Routed probe;
  probe.op = OP_GET; probe.n = n; probe.d_x = d_x; probe.ev_in = ev_in;
  shard_settle_placement(sh, probe, false);
  HIP_OK(hipStreamWaitEvent(s, ev_in, 0));
  uint64_t send[MAX_SHARDS], recv[MAX_SHARDS];
  sh->t_a.need(std::max<size_t>(n, 1));                  // perm
  sh->t_b.need(std::max<size_t>(n, 1) * 2);              // packed {x, x}
  if (smatrix_partition_packed_dev(n, d_x, d_x, nullptr, (uint32_t)R, send, sh->d_work, sh->t_a.p, sh->t_b.p, sh->d_place,
                                   sh->place_slots, sh->d_cuts, s) != 0) smx_die("shard: partition failed");
  std::vector<uint64_t> all((size_t)R * R);
  sh->tr->allgather_host(send, all.data(), (size_t)R * 8, s);
  uint64_t total = 0;
  for (int p = 0; p < R; p++) { recv[p] = all[(size_t)p * R + sh->rank]; total += recv[p]; }
  sh->t_c.need(std::max<uint64_t>(total, 1) * 2);
  sh->tr->alltoallv(sh->t_b.p, send, sh->t_c.p, recv, 2, s);
  sh->t_x.need(std::max<uint64_t>(total, 1)); sh->t_y.need(std::max<uint64_t>(total, 1));
  if (total) {
    smatrix_unpack_dev(total, 2, sh->t_c.p, sh->t_x.p, sh->t_y.p, nullptr, s);
    smatrix_rowlen_batch_dev(sh->local, total, sh->t_x.p, sh->t_y.p, s);     // lengths over the ids' copy
  }
  sh->t_b.need(std::max<size_t>(n, 1) * 2);
  sh->tr->alltoallv(sh->t_y.p, recv, sh->t_b.p, send, 1, s);
  if (n) smatrix_gather_dev(n, sh->t_b.p, sh->t_a.p, d_out, s);
  HIP_OK(hipEventRecord(ev_done, s));
}

void shard_getrow_task(smatrix_shard* sh, size_t n, const uint32_t* d_x, const uint64_t* d_offsets, uint32_t* d_ret, uint32_t* d_counts,
                       hipEvent_t ev_in, hipEvent_t ev_done) {
  hipStream_t s = sh->cs;
  const int R = sh->nranks;
  Routed probe;
  probe.op = OP_GET; probe.n = n; probe.d_x = d_x; probe.ev_in = ev_in;
  shard_settle_placement(sh, probe, false);
  HIP_OK(hipStreamWaitEvent(s, ev_in, 0));
  // records {x, cap}: the owner reads every row into a slot of cap pairs
  uint64_t send[MAX_SHARDS], recv[MAX_SHARDS], psend[MAX_SHARDS], precv[MAX_SHARDS];
  sh->t_y.need(std::max<size_t>(n, 1));                  // caps, caller order
  if (n) hipLaunchKernelGGL(k_caps_from_offsets, dim3(blocks_for(n)), dim3(256), 0, s, (uint32_t)n, d_offsets, sh->t_y.p);
  sh->t_a.need(std::max<size_t>(n, 1));                  // perm
  sh->t_b.need(std::max<size_t>(n, 1) * 2);              // packed {x, cap}
  if (smatrix_partition_packed_dev(n, d_x, sh->t_y.p, nullptr, (uint32_t)R, send, sh->d_work, sh->t_a.p, sh->t_b.p, sh->d_place,
                                   sh->place_slots, sh->d_cuts, s) != 0) smx_die("shard: partition failed");
  std::vector<uint64_t> all((size_t)R * R);
  sh->tr->allgather_host(send, all.data(), (size_t)R * 8, s);
  uint64_t total = 0;
  for (int p = 0; p < R; p++) { recv[p] = all[(size_t)p * R + sh->rank]; total += recv[p]; }
  if (total >= (1ull << 32)) smx_die("sharded getrow: too many rows routed to one rank");
  sh->t_c.need(std::max<uint64_t>(total, 1) * 2);
  sh->tr->alltoallv(sh->t_b.p, send, sh->t_c.p, recv, 2, s);
  // requester side: where the slot of partitioned row q starts (pairs), and how many pairs each owner will send back
  sh->t_off.need(n + 1);
  hipLaunchKernelGGL(k_excl_scan_u32, dim3(1), dim3(1024), 0, s, (uint32_t)n, sh->t_b.p + 1, 2u, sh->t_off.p);
  seg_cap_sums(sh->t_off.p, (uint32_t)n, send, R, precv, s);
  // owner side: offsets over the received caps, the rows, the per-requester slot totals
  sh->t_off2.need(total + 1);
  hipLaunchKernelGGL(k_excl_scan_u32, dim3(1), dim3(1024), 0, s, (uint32_t)total, sh->t_c.p + 1, 2u, sh->t_off2.p);
  seg_cap_sums(sh->t_off2.p, (uint32_t)total, recv, R, psend, s);
  uint64_t slots_out = 0, slots_in = 0;
  for (int p = 0; p < R; p++) { slots_out += psend[p]; slots_in += precv[p]; }
  sh->t_pairs.need(std::max<uint64_t>(slots_out, 1));
  sh->t_pairs2.need(std::max<uint64_t>(slots_in, 1));
  sh->t_x.need(std::max<uint64_t>(total, 1));
  DevBuf<uint32_t>& cnt_owner = sh->t_y;                 // (the caps in caller order are no longer needed)
  cnt_owner.need(std::max<uint64_t>(std::max<uint64_t>(total, n), 1));
  if (total) {
    DevBuf<uint32_t> ids, caps;                          // (ids contiguous for the row kernels)
    ids.need(total); caps.need(total);
    smatrix_unpack_dev(total, 2, sh->t_c.p, ids.p, caps.p, nullptr, s);
    HIP_OK(hipMemsetAsync(cnt_owner.p, 0, total * 4, s));
    smatrix_getrow_batch_dev(sh->local, total, ids.p, sh->t_off2.p, reinterpret_cast<uint32_t*>(sh->t_pairs.p), cnt_owner.p, s);
    HIP_OK(hipStreamSynchronize(s));
    ids.release(); caps.release();
  }
  // back: counts (one word per row), then the slots (two words per pair)
  sh->t_x.need(std::max<size_t>(n, 1));
  sh->tr->alltoallv(cnt_owner.p, recv, sh->t_x.p, send, 1, s);
  sh->tr->alltoallv(reinterpret_cast<const uint32_t*>(sh->t_pairs.p), psend, reinterpret_cast<uint32_t*>(sh->t_pairs2.p), precv, 2, s);
  if (n)
    hipLaunchKernelGGL(k_rows_unpermute, dim3(std::min<uint32_t>(blocks_for((uint64_t)n * 64), 8192)), dim3(256), 0, s, (uint32_t)n, sh->t_a.p,
                       sh->t_x.p, sh->t_off.p, sh->t_pairs2.p, d_offsets, reinterpret_cast<uint64_t*>(d_ret), d_counts);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(ev_done, s));
}

}  // namespace

extern "C" {

int smatrix_shard_unique_id(void* id128) {
  if (transport_is_shm()) {
    // the shm test transport: the id is the name of a fresh shared-memory object
    static std::atomic<uint32_t> seq{0};
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    memset(id128, 0, SMATRIX_SHARD_ID_BYTES);
    snprintf(static_cast<char*>(id128), SMATRIX_SHARD_ID_BYTES, "/smx_shard_%d_%u_%lld", (int)getpid(), seq.fetch_add(1), (long long)ts.tv_nsec);
    return 0;
  }
  if (!g_rccl.load()) return -1;
  ncclUniqueId id;
  if (g_rccl.GetUniqueId(&id) != ncclSuccess) return -1;
  memcpy(id128, &id, sizeof id);
  return 0;
}

smatrix_shard_t* smatrix_shard_open(const char* fname, int rank, int nranks, const void* id128) {
  if (nranks < 1 || nranks > (int)MAX_SHARDS || rank < 0 || rank >= nranks) return nullptr;
  const char* force = getenv("SMATRIX_SHARD_FORCE_RCCL");
  const bool self_over_rccl = force && *force == '1';
  const bool shm = transport_is_shm() && nranks > 1;
  if (nranks > 1 && !id128) return nullptr;
  if (!shm && (nranks > 1 || self_over_rccl) && !g_rccl.load()) return nullptr;
  smatrix_t* local = smatrix_open(fname);
  if (!local) return nullptr;
  smatrix_shard* sh = new smatrix_shard();
  sh->local = local;
  sh->rank = rank;
  sh->nranks = nranks;
  sh->device = M(local)->device;
  if (fname) sh->fname = fname;
  if (const char* a = getenv("SMATRIX_SHARD_PLACE")) sh->auto_place = *a != '0';
  HIP_OK(hipSetDevice(sh->device));
  if (shm) sh->tr = new ShmTransport(rank, nranks, id128);
  else if (nranks > 1 || self_over_rccl) {
    RcclTransport* rt = new RcclTransport(rank, nranks, id128, self_over_rccl);
    if (!rt->failed.empty()) {
      fprintf(stderr, "libsmatrix: shard %d/%d: no RCCL communicator (%s)\n", rank, nranks, rt->failed.c_str());
      delete rt;
      smatrix_close(local);
      delete sh;
      return nullptr;
    }
    sh->tr = rt;
  } else sh->tr = new SelfTransport();
  sh->tr->rank = rank; sh->tr->nranks = nranks;
  dev_malloc(&sh->d_work, 2 * MAX_SHARDS * sizeof(unsigned long long));
  HIP_OK(hipHostMalloc(&sh->h_cnt, 2 * MAX_SHARDS * sizeof(uint64_t)));
  memset(sh->h_cnt, 0, 2 * MAX_SHARDS * sizeof(uint64_t));
  HIP_OK(hipStreamCreateWithFlags(&sh->cs, hipStreamNonBlocking));
  sh->plan.world = nranks;
  // a placement stored next to the shard file (by this library or by libsmatrix_amd/sharded.py): rows ARE where it put them
  if (fname) {
    const std::string pf = sh->fname + ".placement";
    if (FILE* f = fopen(pf.c_str(), "r")) {
      std::string text;
      char buf[4096];
      size_t k;
      while ((k = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, k);
      fclose(f);
      PlacementPlan pl;
      if (!placement_from_json(text, &pl)) smx_die("shard placement: cannot parse the .placement file");
      if (pl.world != nranks) smx_die("shard placement: the stored placement is for another number of shards");
      sh->plan = pl;
      shard_upload_placement(sh);
    }
  }
  sh->comm = std::thread(comm_main, sh);
  return sh;
}

void smatrix_shard_close(smatrix_shard_t* sh) {
  if (!sh) return;
  HIP_OK(hipSetDevice(sh->device));
  {
    std::lock_guard<std::mutex> l(sh->qmu);
    sh->stop = true;
  }
  sh->qcv.notify_all();
  if (sh->comm.joinable()) sh->comm.join();
  (void)hipDeviceSynchronize();
  // the placement goes next to the shard file: rows never move, so a reopen must route the same way
  if (sh->placed || sh->place_dirty) shard_persist_placement(sh);    // (a refresh: it was written when it was decided)
  delete sh->tr;
  for (smatrix_routed& h : sh->pool) {
    Routed& r = h.r;
    for (DevBuf<uint32_t>* b : {&r.perm, &r.packed, &r.recvbuf, &r.res, &r.res2, &r.back, &r.back2}) b->release();
    for (hipEvent_t e : {r.ev_in, r.ev_routed, r.ev_applied, r.ev_done}) if (e) (void)hipEventDestroy(e);
  }
  for (DevBuf<uint32_t>* b : {&sh->t_x, &sh->t_y, &sh->t_a, &sh->t_b, &sh->t_c}) b->release();
  for (DevBuf<uint64_t>* b : {&sh->t_off, &sh->t_off2, &sh->t_pairs, &sh->t_pairs2}) b->release();
  if (sh->cs) (void)hipStreamDestroy(sh->cs);
  if (sh->d_work) (void)hipFree(sh->d_work);
  if (sh->h_cnt) (void)hipHostFree(sh->h_cnt);
  if (sh->d_cuts) (void)hipFree(sh->d_cuts);
  if (sh->d_place) (void)hipFree(sh->d_place);
  smatrix_close(sh->local);
  delete sh;
}

smatrix_t* smatrix_shard_local(smatrix_shard_t* sh) { return sh->local; }
int smatrix_shard_rank(smatrix_shard_t* sh) { return sh->rank; }
int smatrix_shard_nranks(smatrix_shard_t* sh) { return sh->nranks; }
uint64_t smatrix_shard_ops_applied(smatrix_shard_t* sh) { return sh->ops_applied; }
const char* smatrix_shard_transport(smatrix_shard_t* sh) { return sh->tr->name(); }

// include/smatrix_shard.h: which RCCL serves (or would serve) the router in this process -- the path it was mapped from and
// ncclGetVersion(); loads the library the way smatrix_shard_open does.  NULL when none can be loaded.
const char* smatrix_shard_rccl_library(int* version) {
  if (!g_rccl.load()) return nullptr;
  if (version) *version = g_rccl.version;
  return g_rccl.path;
}

int smatrix_shard_set_placement(smatrix_shard_t* sh, const uint32_t* cuts, const uint32_t* place_pairs, uint32_t place_slots) {
  if (place_slots > PLACE_MAX_SLOTS || (place_slots & (place_slots - 1)) || (place_slots && !place_pairs)) return -1;
  std::lock_guard<std::mutex> g(sh->mu);
  PlacementPlan pl;
  pl.world = sh->nranks;
  if (cuts && sh->nranks > 1) { pl.have_cuts = true; pl.cuts.assign(cuts, cuts + sh->nranks - 1); }
  for (uint32_t i = 0; i < place_slots; i++)
    if (place_pairs[2 * i + 1]) {
      if (place_pairs[2 * i + 1] > (uint32_t)sh->nranks) return -1;
      pl.place.push_back({place_pairs[2 * i], place_pairs[2 * i + 1] - 1u});
    }
  // (the device table is sized at twice the rows, shard_upload_placement: more than half of PLACE_MAX_SLOTS do not fit.
  //  Refused here, before the plan is replaced: the handle keeps the placement it had)
  if (pl.place.size() > PLACE_MAX_SLOTS / 2) return -1;
  std::sort(pl.place.begin(), pl.place.end());
  sh->plan = pl;
  sh->placed = true;
  sh->place_dirty = true;
  shard_upload_placement(sh);
  shard_persist_placement(sh);
  return 0;
}

int smatrix_shard_get_placement(smatrix_shard_t* sh, uint32_t* cuts_out, uint32_t* n_cuts, uint32_t* place_pairs_out, uint32_t cap_rows,
                                uint32_t* n_rows) {
  std::lock_guard<std::mutex> g(sh->mu);
  const PlacementPlan& pl = sh->plan;
  if (n_cuts) *n_cuts = pl.have_cuts ? (uint32_t)pl.cuts.size() : 0u;
  if (cuts_out && pl.have_cuts) memcpy(cuts_out, pl.cuts.data(), pl.cuts.size() * 4);
  if (n_rows) *n_rows = (uint32_t)pl.place.size();
  if (place_pairs_out)
    for (uint32_t i = 0; i < std::min<uint32_t>(cap_rows, (uint32_t)pl.place.size()); i++) {
      place_pairs_out[2 * i] = pl.place[i].first;
      place_pairs_out[2 * i + 1] = pl.place[i].second;
    }
  return sh->placed ? 1 : 0;
}

// Host-only face of the planner and of the <file>.placement format (no device, no handle): n {row id, ops} samples of a
// stream of `total` ops -> the plan for `world` shards as the JSON this library stores (and libsmatrix_amd/sharded.py
// reads), written to out (cap bytes, NUL-terminated).  Returns the text's length, or -1 if it does not fit / bad input.
// `reparse` != 0: the text is parsed back and re-serialised first (round trip through placement_from_json).
int smatrix_shard_plan_json(const uint32_t* xs, const uint64_t* counts, size_t n, uint64_t total, int world, int reparse, char* out, size_t cap) {
  if (world < 1 || world > (int)MAX_SHARDS) return -1;
  std::vector<std::pair<uint32_t, uint64_t>> c(n);
  for (size_t i = 0; i < n; i++) c[i] = {xs[i], counts[i]};
  PlacementPlan pl = plan_placement(c, total, world, 256);
  std::string t = placement_to_json(pl);
  if (reparse) {
    PlacementPlan back;
    if (!placement_from_json(t, &back)) return -1;
    t = placement_to_json(back);
  }
  if (t.size() + 1 > cap) return -1;
  memcpy(out, t.c_str(), t.size() + 1);
  return (int)t.size();
}

int smatrix_shard_apply_dev(smatrix_shard_t* sh, int op, size_t n, const uint32_t* d_x, const uint32_t* d_y,
                            const uint32_t* d_v, uint32_t* d_out, void* hip_stream) {
  return shard_apply(sh, op, false, n, d_x, d_y, op == OP_GET ? nullptr : d_v, d_out, nullptr, hip_stream);
}

int smatrix_shard_apply_then_get_dev(smatrix_shard_t* sh, int op, size_t n, const uint32_t* d_x, const uint32_t* d_y,
                                     const uint32_t* d_v, uint32_t* d_out, uint32_t* d_out_get, void* hip_stream) {
  if (op == OP_GET) smx_die("shard: apply-then-get needs a write op");
  return shard_apply(sh, op, true, n, d_x, d_y, d_v, d_out, d_out_get, hip_stream);
}

// ---- split phases (include/smatrix_shard.h) -------------------------------------------------------------------------
smatrix_routed_t* smatrix_shard_route_dev(smatrix_shard_t* sh, int op, size_t n, const uint32_t* d_x, const uint32_t* d_y,
                                          const uint32_t* d_v, int inputs_ready, void* hip_stream) {
  return shard_route(sh, op, n, d_x, d_y, d_v, inputs_ready != 0, static_cast<hipStream_t>(hip_stream));
}
int smatrix_shard_apply_routed(smatrix_shard_t* sh, smatrix_routed_t* h, int then_get, void* hip_stream) {
  shard_apply_routed(sh, h, then_get != 0, static_cast<hipStream_t>(hip_stream));
  return 0;
}
int smatrix_shard_finish(smatrix_shard_t* sh, smatrix_routed_t* h, uint32_t* d_out, uint32_t* d_out_get) {
  shard_finish(sh, h, d_out, d_out_get);
  return 0;
}
int smatrix_shard_wait(smatrix_shard_t* sh, smatrix_routed_t* h, void* hip_stream) {
  shard_wait(sh, h, static_cast<hipStream_t>(hip_stream));
  return 0;
}

// ---- rowlen / getrow of arbitrary rows --------------------------------------------------------------------------------
int smatrix_shard_rowlen_dev(smatrix_shard_t* sh, size_t n, const uint32_t* d_x, uint32_t* d_out, void* hip_stream) {
  if (n >= (1ull << 32)) smx_die("shard: batch too large (n must be < 2^32)");
  std::lock_guard<std::mutex> g(sh->mu);
  HIP_OK(hipSetDevice(sh->device));
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  hipEvent_t ev_in, ev_done;
  HIP_OK(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
  HIP_OK(hipEventCreateWithFlags(&ev_done, hipEventDisableTiming));
  HIP_OK(hipEventRecord(ev_in, s));
  comm_wait(sh, comm_submit(sh, [=] { shard_rowlen_task(sh, n, d_x, d_out, ev_in, ev_done); }));
  HIP_OK(hipStreamWaitEvent(s, ev_done, 0));
  if (!hip_stream) HIP_OK(hipStreamSynchronize(s));
  (void)hipEventDestroy(ev_in); (void)hipEventDestroy(ev_done);
  return 0;
}

int smatrix_shard_getrow_dev(smatrix_shard_t* sh, size_t n, const uint32_t* d_x, const uint64_t* d_offsets, uint32_t* d_ret,
                             uint32_t* d_counts, void* hip_stream) {
  if (n >= (1ull << 32)) smx_die("shard: batch too large (n must be < 2^32)");
  std::lock_guard<std::mutex> g(sh->mu);
  HIP_OK(hipSetDevice(sh->device));
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  hipEvent_t ev_in, ev_done;
  HIP_OK(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
  HIP_OK(hipEventCreateWithFlags(&ev_done, hipEventDisableTiming));
  HIP_OK(hipEventRecord(ev_in, s));
  comm_wait(sh, comm_submit(sh, [=] { shard_getrow_task(sh, n, d_x, d_offsets, d_ret, d_counts, ev_in, ev_done); }));
  HIP_OK(hipStreamWaitEvent(s, ev_done, 0));
  if (!hip_stream) HIP_OK(hipStreamSynchronize(s));
  (void)hipEventDestroy(ev_in); (void)hipEventDestroy(ev_done);
  return 0;
}

}  // extern "C"
