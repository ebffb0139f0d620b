// ------------------------------------------------------------------------------------------------
// Round 4: the 256x256 tile as an 8-phase, two-group ("ping-pong") schedule on v_mfma_f32_16x16x32 fragments.
//
// What changes against gemm_nt256p_kernel (same macro tile, same 8 waves as 2 x 4, same 128x64 per wave, same LDS images and swizzle):
//  * the two waves that share a SIMD (w and w + 4) never want the matrix pipe at the same time.  A K-tile is four PHASES, one 64x32
//    quadrant of the wave's tile each (16 MFMAs on 8 independent accumulators: no dependent back-to-back issue); a phase is
//        LOAD segment: this quadrant's ds_read_b128 fragment reads + the two DMA pieces of one half-tile  -> s_barrier
//        MFMA segment: 16 MFMAs at raised priority                                                     -> s_barrier
//    and the upper wave row (waves 4-7) runs one barrier behind the lower one, so on every SIMD one wave is in its MFMA segment while
//    its partner issues LDS reads and copies -- the pipe sees a continuous MFMA stream instead of two identical streams colliding;
//  * the stage buffers are eight 16 KiB half-tile slots (2 K-tile parities x {A rows 0-127, A 128-255, W 0-127, W 128-255}) refilled one
//    slot per phase as soon as its last reader is two phases behind; ONE counted wait per K-tile (vmcnt(2) at the end of phase 4's LOAD
//    segment: everything but the half-tile just issued has landed), placed one phase before the first read of the data it covers;
//  * the next tile's first K-tile streams in during the current tile's last K-tile, so the K loop runs across tile boundaries without a
//    prologue; the two groups re-align only for the epilogue (both store at the same time) and split again behind it.
// Schedule (K-tile t of the tile, buffer parity P = t & 1; quadrant = (A rows mi*64.., W rows ni*32..) of the wave's 128 x 64):
//    phase 1  reads B(ni 0) + A(mi 0)   copies A-half 0 of K-tile t+1 -> parity P^1     MFMA quadrant (0, 0)
//    phase 2  reads B(ni 1)             copies A-half 1 of K-tile t+1 -> parity P^1     MFMA quadrant (0, 1)
//    phase 3  reads A(mi 1)             copies W-half 1 of K-tile t+1 -> parity P^1     MFMA quadrant (1, 1)
//    phase 4  --                        copies W-half 0 of K-tile t+2 -> parity P, vmcnt(2)   MFMA quadrant (1, 0)
// Hazards (phase index k, barrier b; lower group: LOAD(k) in [b 2k-1, b 2k], MFMA(k) in [2k, 2k+1]; upper group one barrier later):
//    RAW  a wave's wait at the end of LOAD(k) precedes barrier 2k+1 for both groups; the data is first read in LOAD(k+1), after it;
//    WAR  a slot last read in LOAD(kr) is idle once barrier 2kr+2 has passed (the upper group's reads retire inside its MFMA(kr));
//         its refill is issued in LOAD(kw), kw >= kr + 2, i.e. after barrier 2kw-1 >= 2kr+3.  (A-half h: kr = phase 3 of K-tile t-1, kw =
//         phase 1 / 2 of K-tile t; W-half 1: kr = phase 2 of t-1, kw = phase 3 of t; W-half 0: kr = phase 2 of t, kw = phase 4 of t.)
#pragma once
#include "gemm_nt256p_kernels.hpp"   // the same macro tile: BM2, BN2, NT2, EPI_BYTES
namespace alpro {
namespace {
constexpr int HALF2_BYTES = 128 * ROWB;           // 16 KiB: 128 rows x 128 bytes
constexpr int STAGE2_BYTES = 4 * HALF2_BYTES;     // one K-tile parity: A0 | A1 | W0 | W1
typedef __attribute__((address_space(3))) volatile int lds_int_t;

template <typename T, int ACT, int MAP>
__global__ __launch_bounds__(NT2, 2) __attribute__((amdgpu_num_vgpr(127))) void gemm_nt256q_kernel(const alpro_gemm_desc_t g, const TileSched sc) {
  static_assert(sizeof(T) == 2, "16-bit operands only");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int ntn = (g.N + BN2 - 1) / BN2, ntm = (g.M + BM2 - 1) / BM2;
  const int nblk = ntn * ntm;
  const int64_t lda_b = g.lda * 2, ldw_b = g.ldw * 2;
  const int nk = g.K >> 6;                       // K-tiles of 64 elements; even and >= 4 (launcher)
  const uint32_t lds_base = lds_addr_of(smem);

  // ---- which tiles (round 5) ----------------------------------------------------------------------------------------------------
  // Tiles are numbered row-panel-major (tile = tm * ntn + tn) and dealt to the 8 XCDs in chunks of 32: XCD y's LIST is
  //     j -> tile (j / 32) * 256 + y * 32 + (j % 32),        j = 0, 1, 2, ...  while that is < nblk,
  // i.e. the tiles the round-4 static walk (workgroup slot s of 256 takes s, s + 256, ...) gave to the XCD's 32 workgroups, in the order
  // it visited them: at any moment an XCD works on a contiguous run of tiles, so the tn tiles of an A row panel meet in ONE L2.
  //   gemm_sched 0 (sc.blk == nullptr): workgroup idx of the XCD takes j = idx, idx + p, idx + 2p, ... (p = gridDim.x / 8) -- with 256
  //     workgroups exactly that static walk.
  //   gemm_sched 1: the first TWO tiles of a workgroup are the static ones (j = idx, idx + p: no atomic stands between the launch and the first
  //     MFMA); every further j comes from the XCD's ticket counter, j = 2p + ticket: one agent-scope atomic per tile, issued by wave 0 behind
  //     an epilogue two tiles ahead of the tile it pays for and read back behind the next K loop -- nothing is added to the K loop.
  //     A workgroup that cannot be resident -- another kernel holds its CU: RCCL's channels during the overlapped gradient exchange, a side
  //     stream -- draws no tickets: the resident ones finish its share of the lists one tile at a time instead of the launch waiting a whole
  //     extra round for it (profiles/r4_overlap_cu_contention.txt: +42 % with 8 of 256 CUs taken).  Its two STATIC tiles are covered by a
  //     claim word per workgroup: a workgroup claims its own pair with one atomic at its start (the answer is awaited by the pipeline fill's
  //     own wait), and a workgroup that has run out of work -- own list dry: it then looks at all eight counters and all claim words with
  //     ONE pair of loads -- takes tickets of other XCDs' lists and, after those, the pair of a workgroup that has not started yet.
  //     Nobody waits for anybody; the block of counters / claim words is zeroed by the NEXT launch of the same stream (TileSched::prev).
  // Results do not depend on who computes a tile: bitwise identical under either walk.
  const uint32_t p = gridDim.x >> 3;
  const uint64_t t_start = wall_clock64();
  constexpr uint32_t RESCUE_TICKS = 1000;   // 10 us of the 100 MHz wall clock
  auto list_tile = [&](int y, uint32_t j) -> int {
    const uint32_t t = ((j >> 5) << 8) + ((uint32_t)y << 5) + (j & 31u);
    return (j < 0x100000u && t < (uint32_t)nblk) ? (int)t : -1;
  };
  auto list_len = [&](int y) -> int {   // number of valid positions of XCD y's list
    const int rem = (nblk & 255) - 32 * y;
    return (nblk >> 8) * 32 + (rem < 0 ? 0 : (rem > 32 ? 32 : rem));
  };
  // Mailbox wave 0 -> everybody: two dwords at the start of the A-half-1 slot of parity 1.  That slot's last reader is phase 3 of a tile's
  // last K-tile and its next writer the copy of phase 2 of the following tile's first K-tile (two barriers into that tile): dead in between.
  // (an LDS-address-space pointer: through a generic pointer the accesses become FLAT instructions, which count on vmcnt AND lgkmcnt and made
  // every read wait for the epilogue's stores)
  lds_int_t* mbox = (lds_int_t*)(__attribute__((address_space(3))) char*)(smem + STAGE2_BYTES + HALF2_BYTES);
  // walk state (wave 0's copy is the one that counts).  Dynamic: how many XCD lists have run dry for this workgroup (tickets are drawn from
  // XCD (own + wstate) % 8).  Static: the workgroup's next list position.
  uint32_t wstate = sc.blk ? 0u : (uint32_t)(blockIdx.x >> 3) + 2 * p;
  // Tickets a workgroup may still draw AHEAD (pipelined, two tiles before it can start them): its fair share of its own list,
  // ceil((len - 2p) / p).  Without the cap a workgroup that runs a few hundred ns ahead of a neighbour draws the list's last ticket while the
  // neighbour still has two tiles to go, and the launch ends one tile later than the static walk (measured on the qkv shape at B = 64, whose
  // lists divide exactly: +8 %).  Whatever is left when a workgroup is OUT of work -- tickets of workgroups that never started, the other
  // XCDs' lists -- goes through steal(), one tile at a time, to whoever is idle then.
  int quota = 0;
  bool pending = false;   // a pipelined ticket is in flight
  if (sc.blk) {
    const int mine = list_len((int)(blockIdx.x & 7u)) - (int)(2 * p);
    quota = mine > 0 ? (mine + (int)p - 1) / (int)p : 0;
  }
  // One returning atomic, lane 0 of wave 0 only (`on`; otherwise the instruction runs with an empty EXEC mask): `add` = a ticket of the
  // current list's counter, else the claim (atomic or) of workgroup `w`'s word.  The value lands in `r` when the memory system answers:
  // whoever reads it waits first (s_waitcnt vmcnt), like for the copies.  These two forms are for the BLOCKING draws of steal(): `r` is read
  // behind a vmcnt(0) a few instructions on ("+v": one register from the atomic to its reader; a CPU test checks the built ISA).
  auto ticket_issue = [&](uint32_t& r, bool on) {
    uint64_t sv;
    const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane(on ? 1 : 0);
    asm volatile("s_mov_b64 %1, exec\n\ts_mov_b32 exec_lo, %5\n\ts_mov_b32 exec_hi, 0\n\tglobal_atomic_add %0, %2, %3, %4 sc0\n\ts_mov_b64 exec, %1"
                 : "+v"(r), "=&s"(sv) : "v"(((blockIdx.x + wstate) & 7u) * 4u), "v"(1u), "s"(sc.blk), "s"(m) : "memory");
  };
  auto claim_issue = [&](uint32_t& r, uint32_t w, uint32_t bits, bool on) {   // bit 0 / bit 1: the first / second static tile of workgroup w
    uint64_t sv;
    const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane(on ? 1 : 0);
    asm volatile("s_mov_b64 %1, exec\n\ts_mov_b32 exec_lo, %5\n\ts_mov_b32 exec_hi, 0\n\tglobal_atomic_or %0, %2, %3, %4 sc0\n\ts_mov_b64 exec, %1"
                 : "+v"(r), "=&s"(sv) : "v"((SCHED_CLAIM0 + w) * 4u), "v"(bits), "s"(sc.blk), "s"(m) : "memory");
  };
  // The PIPELINED draws (the static pair's claim, the ticket for the tile after next) answer into v255, a register the compiler does not own
  // (the kernel is built with amdgpu_num_vgpr(127): on gfx90a+ the number counts per register-file half, i.e. v0-v253 are the compiler's): their answers are in flight across a pipeline fill / a whole K loop, and a compiler-owned register
  // may be copied or re-assigned at any block boundary in between -- a copy of a register with an atomic in flight copies the OLD contents
  // (it happened whenever an epilogue variant was added: the allocator split the live range).  tk_read() is placed behind a counted wait
  // that was issued after the atomic.
  auto ticket_issue_tk = [&](bool on) {
    uint64_t sv;
    const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane(on ? 1 : 0);
    // reserved-register site (deliberate; -Werror=inline-asm otherwise): v255 is outside the compiler's budget (amdgpu_num_vgpr(127)) and holds the atomic's answer while it is in flight; tests/test_host_cpu.py checks the built ISA (nothing else names v254 / v255, every instantiation is allocated 256 registers)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
    asm volatile("s_mov_b64 %0, exec\n\ts_mov_b32 exec_lo, %4\n\ts_mov_b32 exec_hi, 0\n\tglobal_atomic_add v255, %1, %2, %3 sc0\n\ts_mov_b64 exec, %0"
                 : "=&s"(sv) : "v"(((blockIdx.x + wstate) & 7u) * 4u), "v"(1u), "s"(sc.blk), "s"(m) : "memory", "v255");   // (the clobber is what makes the compiler COUNT v255 into the kernel's register allocation -- without it an instantiation that needs 240 registers gets 240 and the atomic writes outside the wave's file; the "reserved register" warning is expected)
#pragma clang diagnostic pop
  };
  auto claim_issue_tk = [&](uint32_t w, uint32_t bits, bool on) {
    uint64_t sv;
    const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane(on ? 1 : 0);
    // reserved-register site (deliberate; -Werror=inline-asm otherwise): v255 is outside the compiler's budget (amdgpu_num_vgpr(127)) and holds the atomic's answer while it is in flight; tests/test_host_cpu.py checks the built ISA (nothing else names v254 / v255, every instantiation is allocated 256 registers)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
    asm volatile("s_mov_b64 %0, exec\n\ts_mov_b32 exec_lo, %4\n\ts_mov_b32 exec_hi, 0\n\tglobal_atomic_or v255, %1, %2, %3 sc0\n\ts_mov_b64 exec, %0"
                 : "=&s"(sv) : "v"((SCHED_CLAIM0 + w) * 4u), "v"(bits), "s"(sc.blk), "s"(m) : "memory", "v255");   // (the clobber is what makes the compiler COUNT v255 into the kernel's register allocation -- without it an instantiation that needs 240 registers gets 240 and the atomic writes outside the wave's file; the "reserved register" warning is expected)
#pragma clang diagnostic pop
  };
  auto tk_read = [&]() -> uint32_t {   // lane 0's answer (wave 0)
    uint32_t r;
    asm volatile("v_readfirstlane_b32 %0, v255" : "=s"(r) : : "memory");
    return r;
  };
  // ticket -> tile of the list tickets are currently drawn from; a dry list moves the workgroup on to the next XCD's
  auto ticket_tile = [&](uint32_t k) -> int {
    int t;
    if (sc.blk) {
      t = list_tile((int)((blockIdx.x + wstate) & 7u), 2 * p + k);
      if (t < 0) ++wstate;
    } else {
      t = list_tile((int)(blockIdx.x & 7u), wstate);
      wstate += p;
    }
    return t;
  };
  // A workgroup out of work (dynamic walk; every wave calls it, one barrier; no copy in flight: the caller drained vmcnt).  Wave 0 reads the
  // eight counters and the claim words (five loads in flight together), then
  //   * takes ONE ticket of the first list (own XCD's first) that still has positions left -- one, not a pair: the last partial round then
  //     spreads over everybody who is out of work instead of the first arrivals taking two tiles each --, or, when every list is dry,
  //   * claims ONE static tile nobody has claimed yet (a workgroup that could not start: some other kernel holds its CU).  Which one is drawn
  //     from a hash of the workgroup id over all open tiles, so that a few hundred helpers arriving together do not all go for the same word.
  //     Rescue waits until RESCUE_TICKS after this workgroup's own start (`t_start`, 100 MHz wall clock): by then every workgroup that CAN be
  //     resident has started and claimed its pair (a later rescue of a workgroup that starts at that very moment is still correct: the claim
  //     atomic arbitrates; it only costs that workgroup its pipeline fill),
  // and posts the tile (-1: nothing left anywhere).  A ticket that comes back beyond its list, or a claim somebody else won, means the picture
  // was stale: look again.
  auto steal = [&](int& t0, int& t1) {
    if (wave == 0) {
      int a = -1;
      for (int tries = 0; tries < 96 && a < 0; ++tries) {
        const uint32_t cnt = lane < 8 ? __hip_atomic_load(sc.blk + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        u32x4 clm;   // claim words of workgroups 4 lane .. 4 lane + 3 (agent-scope loads: the words are set by other XCDs' atomics)
        clm.x = __hip_atomic_load(sc.blk + SCHED_CLAIM0 + 4 * lane + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        clm.y = __hip_atomic_load(sc.blk + SCHED_CLAIM0 + 4 * lane + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        clm.z = __hip_atomic_load(sc.blk + SCHED_CLAIM0 + 4 * lane + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        clm.w = __hip_atomic_load(sc.blk + SCHED_CLAIM0 + 4 * lane + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int y = -1;
        for (int i = 0; i < 8 && y < 0; ++i) {
          const int c = (int)((blockIdx.x + i) & 7u);
          if ((int)__builtin_amdgcn_readlane(cnt, c) < list_len(c) - (int)(2 * p)) y = c;
        }
        if (y >= 0) {
          uint32_t k0 = 0;
          wstate = (uint32_t)((y - (int)(blockIdx.x & 7u)) & 7);   // tickets are drawn from (own + wstate) % 8 from here on
          ticket_issue(k0, true);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          a = list_tile(y, 2 * p + __builtin_amdgcn_readfirstlane(k0));
          continue;
        }
        // open static tiles: slot s = 2 i + b of a lane is tile b (0 = first, 1 = second) of workgroup 4 lane + i; workgroups below gridDim.x count
        const uint32_t w0 = 4u * lane;
        const uint32_t words[4] = {clm.x, clm.y, clm.z, clm.w};
        uint64_t open[8];
        int total = 0;
#pragma unroll
        for (int sl = 0; sl < 8; ++sl) {
          open[sl] = __builtin_amdgcn_ballot_w64(w0 + (sl >> 1) < gridDim.x && ((words[sl >> 1] >> (sl & 1)) & 1u) == 0u);
          total += __builtin_popcountll(open[sl]);
        }
        if (total == 0) break;
        while ((uint32_t)(wall_clock64() - t_start) < RESCUE_TICKS) __builtin_amdgcn_s_sleep(8);
        int q = (int)(((blockIdx.x + 1u) * 0x9E3779B1u >> 12) % (uint32_t)total);   // the q-th open tile, q spread over the helpers
        uint32_t w = 0, bit = 0;
#pragma unroll
        for (int sl = 0; sl < 8; ++sl) {
          const int n = __builtin_popcountll(open[sl]);
          if (bit == 0 && q < n) {
            uint64_t msk = open[sl];
            for (int i = 0; i < q; ++i) msk &= msk - 1;
            w = 4u * (uint32_t)__builtin_ctzll(msk) + (uint32_t)(sl >> 1);
            bit = 1u << (sl & 1);
          }
          q -= n;
        }
        uint32_t old = 3;
        claim_issue(old, w, bit, true);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if ((__builtin_amdgcn_readfirstlane(old) & bit) == 0) a = list_tile((int)(w & 7u), (w >> 3) + (bit == 2u ? p : 0u));   // (-1: that workgroup had no such tile -- look again)
      }
      const int b = -1;
      mbox[0] = a;
      mbox[1] = b;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    t0 = __builtin_amdgcn_readfirstlane(mbox[0]);
    t1 = __builtin_amdgcn_readfirstlane(mbox[1]);
  };

  // DMA sources.  Nothing is clamped per lane and everything tile-dependent is wave-uniform: a copy reads
  //   [A + (m0 + h*128) * lda_b + kt*128]  (SGPR pair)  +  [((r0 + i*8) * lda_b + chunk*16) ^ i*64]  (one 32-bit VGPR per piece)
  // for piece i of half-tile h, r0 = wave*16 + (lane >> 3) = the lane's row in piece 0, chunk = (lane & 7) ^ swizzle(r0); piece 1 sits 8 rows
  // further, where the swizzle differs by 4 chunks = 64 bytes (lda_b is a multiple of 128: launcher).
  const int r0 = wave * 16 + (lane >> 3);
  const uint32_t sw0 = (uint32_t)(((lane & 7) ^ ((r0 >> 1) & 7)) << 4);
  uint32_t oa[2], ow[2][2];   // A: [piece i] (the half-tile's 128 rows sit in its base pointer); W: [half-tile h][piece i]: the lane's byte offset
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    oa[i] = (uint32_t)((r0 + i * 8) * lda_b) + (sw0 ^ (uint32_t)(i * 64));
#pragma unroll
    for (int h = 0; h < 2; ++h) ow[h][i] = (uint32_t)((r0 + h * 128 + i * 8) * ldw_b) + (sw0 ^ (uint32_t)(i * 64));
  }
  // Tile bases (wave-uniform).  a[h] = where THIS WAVE's 16 rows of A half-tile h start, minus the wave's own row offset (which oa carries):
  // normally A + (m0 + h * 128) * lda_b.  Ragged last tile row (M % 256 = vr valid rows, a multiple of 16: launcher): a wave's two copy
  // instructions per half-tile move rows [h * 128 + wave * 16, + 16) -- valid or not as a whole -- and an invalid group re-reads rows 0-15 of
  // the tile instead (base moved back by wave * 16 rows): finite values that only reach accumulator rows the epilogue never stores.  All of it
  // is folded into the per-tile base: the copies in the K loop cost what they cost on a full tile.
  struct Tile { const char* a[2]; const char* w; };
  auto tile_base = [&](int tile) {
    const int tm = ntn == 1 ? tile : (int)__umulhi((uint32_t)tile, sc.magic_ntn), tn = tile - tm * ntn;
    const int vr = g.M - tm * BM2;   // (>= 256 on full tiles)
    const char* a0 = (const char*)g.A + (int64_t)tm * BM2 * lda_b;
    Tile t;
#pragma unroll
    for (int h = 0; h < 2; ++h) t.a[h] = a0 + (int64_t)((h * 128 + wave * 16 < vr) ? h * 128 : -(wave * 16)) * lda_b;
    t.w = (const char*)g.W + (int64_t)tn * BN2 * ldw_b;
    return t;
  };
  // half-tile `hs` (0 / 1: A rows 0-127 / 128-255, 2 / 3: W rows) from `kbase` (= that half's tile base + kt * 128 bytes, wave-uniform) -> slot hs of parity `par`
  auto copy_half = [&](const char* kbase, int hs, int par) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const uint32_t vo = hs < 2 ? oa[i] : ow[hs & 1][i];
      dma16_sbase(vo, kbase, __builtin_amdgcn_readfirstlane(lds_base + par * STAGE2_BYTES + hs * HALF2_BYTES + (wave * 2 + i) * 1024));
    }
  };
  // fragment read offsets: lane l supplies row (l & 15) and the 8-element k group (l >> 4) of a 16 x 32 operand fragment; chunk index
  // (ks * 4 + kg) ^ swizzle(row) == (ks * 64 bytes) ^ ((kg ^ swizzle) * 16 bytes)
  const int l15 = lane & 15, kg = lane >> 4;
  const int frag0 = l15 * ROWB + ((kg ^ ((l15 >> 1) & 7)) << 4);
  const char* aF[2] = {smem + wr * HALF2_BYTES + frag0, smem + wr * HALF2_BYTES + (frag0 ^ 64)};
  const char* bF[2] = {smem + (2 + (wc >> 1)) * HALF2_BYTES + (wc & 1) * 64 * ROWB + frag0,
                       smem + (2 + (wc >> 1)) * HALF2_BYTES + (wc & 1) * 64 * ROWB + (frag0 ^ 64)};
  float* stage = (float*)(smem + 2 * STAGE2_BYTES + wave * (16 * 64 * 4));   // 4 KiB per wave: 16 rows x 64 columns fp32

  // (the ticket in flight -- lane 0 of wave 0, v255: drawn behind tile i - 1's epilogue for tile i + 2, read back behind tile i's K loop)
  // the static pair, and (dynamic walk) its claim: in flight under the pipeline fill.  Workgroup 0 also hands the block of this stream's
  // PREVIOUS launch back zeroed (that launch is complete: same stream).
  int cur_t = list_tile((int)(blockIdx.x & 7u), blockIdx.x >> 3), nxt_t = list_tile((int)(blockIdx.x & 7u), (blockIdx.x >> 3) + p);
  if (sc.prev && blockIdx.x == 0 && wave == 0) {
#pragma unroll
    for (int i = 0; i < (SCHED_BLOCK_U32 + 63) / 64; ++i)
      if (i * 64 + lane < SCHED_BLOCK_U32) sc.prev[i * 64 + lane] = 0u;
  }
  claim_issue_tk(blockIdx.x, 3u, wave == 0 && sc.blk);   // (the answer travels in the ticket register: the first ticket is drawn after it has been read)
  bool fresh = sc.blk != nullptr;   // the static pair's claim is in flight
  bool have = cur_t >= 0;
  while (true) {
  if (!have) {
    if (!sc.blk) break;
    fresh = false;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (steal()'s own waits count on an empty queue)
    steal(cur_t, nxt_t);
    if (cur_t < 0) break;
    quota = 0;   // from here on one tile at a time, when idle
  }
  have = false;
  Tile cur = tile_base(cur_t);
  Tile nxt = tile_base(nxt_t >= 0 ? nxt_t : cur_t);   // (no next tile: the run-ahead copies re-read this tile's first K-tiles into dead slots)
  // pipeline fill: K-tile 0 complete in parity 0, W-half 0 of K-tile 1 on its way into parity 1
#pragma unroll
  for (int hs = 0; hs < 4; ++hs) copy_half(hs < 2 ? cur.a[hs] : cur.w, hs, 0);
  copy_half(cur.w + ROWB, 2, 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (fresh && wave == 0) {   // are the static tiles still this workgroup's?  (wave 0's wait above covered the claim)
    mbox[0] = (int)(tk_read() & 3u);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  phase_barrier();
  if (fresh) {
    fresh = false;
    const int gone = __builtin_amdgcn_readfirstlane(mbox[0]);   // bit 0 / 1: somebody rescued the first / second one while this workgroup waited for a CU
    if (gone) {
      phase_barrier();   // (everybody has read the mailbox before it is written again)
      int t0 = (gone & 1) ? -1 : cur_t, t1 = (gone & 2) ? -1 : nxt_t;
      if (t0 < 0) { t0 = t1; t1 = -1; }
      cur_t = t0;
      nxt_t = t1;
      have = cur_t >= 0;
      continue;   // fill the pipeline again for what is left, or look for other work
    }
  }
  pending = sc.blk && nxt_t >= 0 && quota > 0;
  quota -= pending ? 1 : 0;
  ticket_issue_tk(wave == 0 && pending);   // for the tile after next

  while (true) {
    const int tile = cur_t;
    const int tm0 = (ntn == 1 ? tile : (int)__umulhi((uint32_t)tile, sc.magic_ntn)) * BM2, tn0 = (tile - (tm0 >> 8) * ntn) * BN2;
    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (wr == 1) phase_barrier();   // the upper wave row drops one barrier behind

    // one K-tile (parity P compile-time): four phases
    auto ktile = [&](auto par_tag, int t) {
      constexpr int P = decltype(par_tag)::value;
      u32x4 fa[4][2], fb[2][2][2];
      const bool in1 = t + 1 < nk, in2 = t + 2 < nk;          // targets inside this tile? else the next tile's K-tile 0 / 1
      const int k1 = in1 ? t + 1 : 0, k2 = in2 ? t + 2 : t + 2 - nk;
      const char* a10 = (in1 ? cur.a[0] : nxt.a[0]) + (int64_t)k1 * ROWB;   // K-tile t+1: both A halves and W half 1
      const char* a11 = (in1 ? cur.a[1] : nxt.a[1]) + (int64_t)k1 * ROWB;
      const char* w1 = (in1 ? cur.w : nxt.w) + (int64_t)k1 * ROWB;
      const char* w2 = (in2 ? cur.w : nxt.w) + (int64_t)k2 * ROWB;   // K-tile t+2: W half 0
      auto load_a = [&](int mi) {
#pragma unroll
        for (int f = 0; f < 4; ++f)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) fa[f][ks] = *(const u32x4*)(aF[ks] + P * STAGE2_BYTES + (mi * 64 + f * 16) * ROWB);
      };
      auto load_b = [&](int ni) {
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) fb[ni][f][ks] = *(const u32x4*)(bF[ks] + P * STAGE2_BYTES + (ni * 32 + f * 16) * ROWB);
      };
      auto mma = [&](int mi, int ni) {
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int f = 0; f < 4; ++f)
#pragma unroll
            for (int e = 0; e < 2; ++e) acc[mi * 4 + f][ni * 2 + e] = Mma16<T>::run(fa[f][ks], fb[ni][e][ks], acc[mi * 4 + f][ni * 2 + e]);
        __builtin_amdgcn_s_setprio(0);
      };
      // phase 1
      load_b(0);
      load_a(0);
      copy_half(a10, 0, P ^ 1);
      phase_barrier();
      mma(0, 0);
      phase_barrier();
      // phase 2
      load_b(1);
      copy_half(a11, 1, P ^ 1);
      phase_barrier();
      mma(0, 1);
      phase_barrier();
      // phase 3
      load_a(1);
      copy_half(w1, 3, P ^ 1);
      phase_barrier();
      mma(1, 1);
      phase_barrier();
      // phase 4
      copy_half(w2, 2, P);
      asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      phase_barrier();
      mma(1, 0);
      phase_barrier();
    };
    for (int t = 0; t < nk; t += 2) {
      ktile(std::integral_constant<int, 0>{}, t);
      ktile(std::integral_constant<int, 1>{}, t + 1);
    }
    // Where the NEXT ticket is drawn.  Behind the epilogue it has ~2 us until the next K loop's first counted wait, which is in-order: it also
    // waits for this atomic, and 32 workgroups of an XCD that run in lockstep hit their counter together.  An epilogue without loads has no
    // wait of its own behind its first fragment row (the bias values are the only thing it fetches), so there the ticket goes out right
    // behind that row (another ~3 us of slack); the epilogues that fetch rows all along (saved factor, fp32 residual: their counted waits
    // would stall on the atomic) keep drawing behind themselves.  (Measured effect of the early draw: within noise.  Of the +6 % of the B = 64
    // qkv shape it was introduced against, half was the first-measurement-of-the-process artefact of the probe -- clocks still settling,
    // profiles/r5_gemm_stagger_probe.txt -- and +3 % is still there on that shape with a warm-up: profiles/r5_gemm_sched_contention.txt.)
    constexpr bool EPI_LOADS = ACT == ALPRO_ACT_GELU_BWD || ACT == ALPRO_ACT_MUL_SAVED;
    constexpr bool PK_ACT = MAP == ALPRO_MAP_IDENTITY && (ACT == ALPRO_ACT_NONE || ACT == ALPRO_ACT_GELU || ACT == ALPRO_ACT_RELU || ACT == ALPRO_ACT_GELU_SAVE_GRAD ||
                                                        ACT == ALPRO_ACT_MUL_SAVED);
    // (the saved-factor multiply takes it only when the factor lies in the tile layout -- c2_tiled, below; the launcher refuses a tiled
    // descriptor this test would send down the staged path)
    const bool pk = PK_ACT && (sc.epi != 0 || g.c2_tiled) && g.c_dtype != ALPRO_F32 && !g.residual && !g.row_scale && !g.drop_seed &&
                    (ACT == ALPRO_ACT_GELU_SAVE_GRAD || (ACT == ALPRO_ACT_MUL_SAVED ? g.c2_tiled != 0 : !g.C2));
    const bool early = !EPI_LOADS && !g.residual;
    int nn_w0 = -1;
    if (wave == 0) {   // the tile after next: the ticket drawn a tile ago has landed (every counted wait of this K loop was issued behind it)
      nn_w0 = (pending || (!sc.blk && nxt_t >= 0)) ? ticket_tile(tk_read()) : -1;   // (no ticket drawn / a dry list: -1 -- steal() behind the next tile looks further)
      mbox[0] = nn_w0;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    auto early_ticket = [&] {   // wave 0, behind the first fragment row of a load-free epilogue
      if (wave == 0 && early) {
        pending = sc.blk && nn_w0 >= 0 && nxt_t >= 0 && quota > 0;
        quota -= pending ? 1 : 0;
        ticket_issue_tk(pending);
      }
    };
    if (wr == 0) phase_barrier();   // re-align: both wave rows run their epilogues at the same time

    // ---- epilogue: one 16-row fragment row (16 x 64 fp32 = 4 KiB of wave-private LDS) at a time
    {
      // The epilogue's own copy of the lane id, opaque to the optimiser: everything lane-derived below (staging offsets, row / column pieces,
      // output pointers) is then computed HERE, where the 64 fragment registers are free -- hoisted over the K loop as tile-loop invariants
      // they were spilled at kernel start and reloaded per fragment row (a scratch load returns behind every store issued before it).
      int le = lane;
      asm volatile("" : "+v"(le));
      const int l15 = le & 15, kg = le >> 4;
      const int mb = tm0 + wr * 128, nb = tn0 + wc * 64;
      auto rows_ok = [&](int mf) { return mb + mf * 16 < g.M; };   // (wave-uniform)
      auto stage_rows = [&](int mf) {
        wave_lds_order();   // the other lanes' reads of the previous fragment row are issued before these writes ...
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
#pragma unroll
          for (int r = 0; r < 4; ++r) stage[(kg * 4 + r) * 64 + nf * 16 + l15] = acc[mf][nf][r];
        wave_lds_order();   // ... and every write of this one before the reads that follow
      };
      if (g.c_dtype != ALPRO_F32) {
        if constexpr (MAP == ALPRO_MAP_IDENTITY) {
          constexpr bool READS_C2 = ACT == ALPRO_ACT_GELU_BWD || ACT == ALPRO_ACT_MUL_SAVED;
          // The PACKED path (round 5): bias / activation / conversion to 16 bits happen in the accumulator layout, and what crosses the LDS is
          // the 16-bit result -- two fragment rows (32 x 64) per pass as 8-byte units of four rows x one column, one ds_write_b64 per
          // fragment instead of four ds_write_b32 (the staging writes are what an epilogue costs first: 128 ds_write_b32 per wave at 4 LDS
          // cycles each = 2 us per tile, all eight waves on the one LDS pipe), four ds_read_b128 per lane (8 columns x 4 rows) and 16 v_perm
          // to turn them into four 16-byte row pieces.  For the epilogues that need nothing in the OUTPUT layout: no residual, row scale,
          // dropout or saved factor, full fragment rows.  The 16-byte pieces of a 64-byte block are XORed with the row group so that the 16
          // lanes of a ds_read_b128 group hit 16 different slots.  Same values as the staged fp32 path (every step is elementwise).
          if (pk && mb >= g.M) {
            // (a wave of the last tile row without a valid row)
          } else if (pk) {
            if constexpr (PK_ACT) {
              typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
              typedef __attribute__((address_space(3))) char lds_char_t;
              lds_char_t* st8 = (lds_char_t*)(smem + 2 * STAGE2_BYTES) + wave * (16 * 64 * 4);
              float bcol[4];
#pragma unroll
              for (int nf = 0; nf < 4; ++nf) bcol[nf] = g.bias ? g.bias[nb + nf * 16 + l15] : 0.f;
              const int kgx = le >> 3, cg = le & 7;
              const int woff = kg * 512 + (l15 >> 3) * 64 + ((((l15 >> 1) & 3) ^ kg) << 4) + (l15 & 1) * 8;   // + f * 2048 + nf * 128
              const int roff = kgx * 512 + cg * 64;                                                            // + ((j ^ (kgx & 3)) << 4)
              const int64_t ldc = g.ldc, ldc2 = g.ldc2;
              T* Cb = (T*)g.C + (int64_t)(mb + 4 * kgx) * ldc + nb + 8 * cg;
              T* C2b = ACT == ALPRO_ACT_GELU_SAVE_GRAD ? (T*)g.C2 + (int64_t)(mb + 4 * kgx) * ldc2 + nb + 8 * cg : nullptr;
              // The saved factor in the TILE layout (c2_tiled; gelu' of fc1, written by the GELU_SAVE_GRAD form and read back by the MUL_SAVED
              // dgrad of fc2 -- nobody else looks at it): element (fragment row mf, fragment nf, row r of the lane's four, lane) of wave w of
              // tile t lives at ((t * 8 + w) * 8 + mf) * 1024 + (nf >> 1) * 512 + lane * 8 + (nf & 1) * 4 + r -- i.e. exactly the accumulator
              // registers, 16 bits each, two 16-byte pieces per lane and fragment row, 1 KiB contiguous per store / load instruction.  Neither
              // kernel sends it through the LDS, and the dgrad multiplies in fp32 BEFORE the conversion, like the staged path does.
              T* C2t = (ACT == ALPRO_ACT_GELU_SAVE_GRAD || ACT == ALPRO_ACT_MUL_SAVED) ? (T*)g.C2 + ((int64_t)tile * 8 + wave) * 8192 + le * 8 : nullptr;
              const int rows_here = g.M - mb;   // (> 0: waves without a valid row do not get here; >= 128 on all but the last tile row)
              auto drain = [&](T* base, int64_t ld, int u) {   // the staged 32 x 64 block -> four row pieces per lane
                u32x4 q[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) q[j] = *(const __attribute__((address_space(3))) u32x4*)(st8 + roff + ((j ^ (kgx & 3)) << 4));
                wave_lds_order();
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const u32x4 o = units_to_row(q, r);
                  if (32 * u + 4 * kgx + r < rows_here) __builtin_nontemporal_store(o, (u32x4*)(base + (int64_t)(32 * u + r) * ld));
                }
              };
              constexpr bool MULS = ACT == ALPRO_ACT_MUL_SAVED;
              // saved-factor passes in flight: two buffers of 16 registers; pass u + 2 is requested into pass u's buffer as soon as pass u's
              // products are formed, i.e. 1.5 passes (~1.5 us) ahead of its use (a third buffer spills accumulators at the path's entry)
              constexpr int PDU = 2, RINGU = MULS ? 2 : 1;
              u32x4 sring[RINGU][2][2];
              auto load_saved = [&](int u, u32x4(&ss)[2][2]) {
#pragma unroll
                for (int f = 0; f < 2; ++f)
#pragma unroll
                  for (int j = 0; j < 2; ++j) ss[f][j] = __builtin_nontemporal_load((const u32x4*)(C2t + (2 * u + f) * 1024 + j * 512));
              };
              if constexpr (MULS) {
#pragma unroll
                for (int u = 0; u < PDU; ++u) load_saved(u, sring[u]);
              }
              const bool tiled = g.c2_tiled != 0;
#pragma unroll
              for (int u = 0; u < 4; ++u) {
                u32x2_t dpk[2][4];
                wave_lds_order();
#pragma unroll
                for (int f = 0; f < 2; ++f)
#pragma unroll
                  for (int nf = 0; nf < 4; ++nf) {
                    float v[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = g.alpha * acc[2 * u + f][nf][r] + bcol[nf];
                    if constexpr (ACT == ALPRO_ACT_GELU_SAVE_GRAD) {
                      f32x2v y0, d0, y1, d1;
                      gelu_and_grad2((f32x2v){v[0], v[1]}, y0, d0);
                      gelu_and_grad2((f32x2v){v[2], v[3]}, y1, d1);
                      v[0] = y0.x; v[1] = y0.y; v[2] = y1.x; v[3] = y1.y;
                      dpk[f][nf] = (u32x2_t){pack2(d0.x, d0.y, (T*)0), pack2(d1.x, d1.y, (T*)0)};
                    } else if constexpr (ACT == ALPRO_ACT_GELU) {
                      const f32x2v y0 = gelu_fast2((f32x2v){v[0], v[1]}), y1 = gelu_fast2((f32x2v){v[2], v[3]});
                      v[0] = y0.x; v[1] = y0.y; v[2] = y1.x; v[3] = y1.y;
                    } else if constexpr (MULS) {
                      const u32x4& sv = sring[u % RINGU][f][nf >> 1];
                      float pre[4];
                      unpack_pair<T>((nf & 1) ? sv.z : sv.x, pre[0], pre[1]);
                      unpack_pair<T>((nf & 1) ? sv.w : sv.y, pre[2], pre[3]);
#pragma unroll
                      for (int r = 0; r < 4; ++r) v[r] *= pre[r];
                    } else {
#pragma unroll
                      for (int r = 0; r < 4; ++r) v[r] = apply_act<T, ACT>(v[r]);
                    }
                    *(__attribute__((address_space(3))) u32x2_t*)(st8 + woff + f * 2048 + nf * 128) = (u32x2_t){pack2(v[0], v[1], (T*)0), pack2(v[2], v[3], (T*)0)};
                  }
                wave_lds_order();
                if constexpr (MULS) {
                  if (u + PDU < 4) load_saved(u + PDU, sring[u % RINGU]);
                }
                drain(Cb, ldc, u);
                if constexpr (ACT == ALPRO_ACT_GELU_SAVE_GRAD) {
                  if (tiled) {
#pragma unroll
                    for (int f = 0; f < 2; ++f)
#pragma unroll
                      for (int j = 0; j < 2; ++j)
                        __builtin_nontemporal_store(mk4(dpk[f][2 * j].x, dpk[f][2 * j].y, dpk[f][2 * j + 1].x, dpk[f][2 * j + 1].y), (u32x4*)(C2t + (2 * u + f) * 1024 + j * 512));
                  } else {
#pragma unroll
                    for (int f = 0; f < 2; ++f)
#pragma unroll
                      for (int nf = 0; nf < 4; ++nf) *(__attribute__((address_space(3))) u32x2_t*)(st8 + woff + f * 2048 + nf * 128) = dpk[f][nf];
                    wave_lds_order();
                    drain(C2b, ldc2, u);
                  }
                }
                if (u == 0) early_ticket();
              }
            }
          } else {
          float bias8[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) bias8[e] = g.bias ? g.bias[nb + (le & 7) * 8 + e] : 0.f;
          // The saved-factor rows (MUL_SAVED: gelu' of the forward, 16 bits) are fetched PD fragment rows ahead of their use.  A fragment row of
          // the epilogue takes ~0.5 us and an HBM round trip 1-2 us: with one row of run-ahead (round 4) every row waited for its loads -- the
          // whole gap between this dgrad (0.34 of peak in the step) and the plain 16-bit-output GEMM (0.40).  The ring lives in the registers the
          // K loop's fragments occupied (64 of them are free here): PD = 2 -> 3 x 8 registers (PD = 3 spills).
          constexpr int PD = 2, RING = PD + 1;
          u32x4 pring[RING][2];
          auto load_pre = [&](int mf, u32x4(&pp)[2]) {
#pragma unroll
            for (int p = 0; p < 2; ++p)
              pp[p] = __builtin_nontemporal_load((const u32x4*)((const T*)g.C2 + (int64_t)(mb + mf * 16 + p * 8 + (le >> 3)) * g.ldc2 + nb + (le & 7) * 8));
          };
          if (READS_C2) {
#pragma unroll
            for (int mf = 0; mf < PD; ++mf)
              if (rows_ok(mf)) load_pre(mf, pring[mf]);
          }
          auto rows_loop = [&](auto res_tag) {
            constexpr bool RES = decltype(res_tag)::value;
#pragma unroll
            for (int mf = 0; mf < 8; ++mf) {
              if (!rows_ok(mf)) break;   // ragged last tile row: fragment rows at or beyond M are not stored (M % 16 == 0: launcher)
              if (READS_C2 && mf + PD < 8 && rows_ok(mf + PD)) load_pre(mf + PD, pring[(mf + PD) % RING]);
              stage_rows(mf);
              epi_rows16_c16<T, ACT, 2, RES>(g, stage, mb + mf * 16, nb, le, bias8, READS_C2 ? pring[mf % RING] : nullptr);
              if constexpr (!RES && !READS_C2) {
                if (mf == 0) early_ticket();
              }
            }
          };
          if (g.residual) rows_loop(std::true_type{});   // (see epi_rows16_c16: no conditional vector load inside the passes)
          else rows_loop(std::false_type{});
          }
        }
      }
      // fp32 output (launcher: ACT none, identity map, no C2 / dropout): C = residual + row_scale * (alpha * acc + bias) -- the MLP's fc2 with its
      // fp32 residual (vit.py:212).  A staged fragment row is 16 rows x 16 float4; lane l finishes pieces l, l+64, l+128, l+192 = rows
      // (l >> 4) + 4j, columns 4 (l & 15) .. +3: whole 256-byte row segments per 16 lanes, the residual pieces of the NEXT fragment row in flight.
      if constexpr (MAP == ALPRO_MAP_IDENTITY && ACT == ALPRO_ACT_NONE) {
        if (g.c_dtype == ALPRO_F32) {
          const int c4 = (le & 15) * 4, r0e = le >> 4;
          float bias4[4];
          load_bias4(g, nb + c4, bias4);
          float* Cf = (float*)g.C;
          // Round 5: the residual rows run PD fragment rows ahead in a register ring and the row scales come WITHOUT a branch inside the
          // row loop.  (Round 4 held one row of run-ahead and a conditional row-scale load per row: the join behind it is closed with
          // s_waitcnt vmcnt(0), so every fragment row waited for the residual rows just requested AND for its predecessor's stores.)
          // The row scale of a fragment row: its 16 rows span at most two groups when row_scale_group >= 16 (the drop-path scale of fc2:
          // one value per clip of 1569 rows) -- one scalar division per fragment row, one or two scalar loads, a compare per row.
          constexpr int PD = 1, RING = PD + 1;   // (two rows ahead do not fit: 48 registers next to the 128 accumulators spill into the row loop)
          f32x4 ring[RING][4];
          auto load_res = [&](int mf, f32x4(&rr)[4]) {
#pragma unroll
            for (int j = 0; j < 4; ++j) rr[j] = __builtin_nontemporal_load((const f32x4*)(g.residual + (int64_t)(mb + mf * 16 + r0e + 4 * j) * g.ldr + nb + c4));
          };
          auto f32_rows = [&](auto res_tag) {
            constexpr bool HAS_RES = decltype(res_tag)::value;
            if constexpr (HAS_RES) {
#pragma unroll
              for (int mf = 0; mf < PD; ++mf)
                if (rows_ok(mf)) load_res(mf, ring[mf]);
            }
#pragma unroll
            for (int mf = 0; mf < 8; ++mf) {
              if (!rows_ok(mf)) break;
              if constexpr (HAS_RES) {
                if (mf + PD < 8 && rows_ok(mf + PD)) load_res(mf + PD, ring[(mf + PD) % RING]);
              }
              float rs_lo = 1.0f, rs_hi = 1.0f;
              uint32_t edge = 0;   // first row (absolute, with m_off; rows < 2^31) of the second group
              if (g.row_scale) {   // scalar loads (wave-uniform addresses): no vector-memory join
                const uint32_t m0 = (uint32_t)g.m_off + (uint32_t)(mb + mf * 16);
                const uint32_t gi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(m0 / (uint32_t)g.row_scale_group));
                edge = (gi + 1) * (uint32_t)g.row_scale_group;
                rs_lo = sload_f32(g.row_scale, gi);
                rs_hi = sload_f32(g.row_scale, edge < (uint32_t)g.m_off + (uint32_t)g.M ? gi + 1 : gi);
              }
              stage_rows(mf);
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const int row = r0e + 4 * j;
                const int64_t m = mb + mf * 16 + row;
                const float4 a = *(const float4*)(stage + row * 64 + c4);
                const float rs = ((uint32_t)g.m_off + (uint32_t)m) >= edge ? rs_hi : rs_lo;   // (no row scale: both are 1)
                f32x4 v = {(g.alpha * a.x + bias4[0]) * rs, (g.alpha * a.y + bias4[1]) * rs, (g.alpha * a.z + bias4[2]) * rs, (g.alpha * a.w + bias4[3]) * rs};
                if constexpr (HAS_RES) v += ring[mf % RING][j];
                __builtin_nontemporal_store(v, (f32x4*)(Cf + m * g.ldc + nb + c4));
              }
              if constexpr (!HAS_RES) {
                if (mf == 0) early_ticket();
              }
            }
          };
          // (row_scale_group < 16 would need a scale per row: not a shape of this model -- the launcher keeps such descriptors off this kernel)
          if (g.residual) f32_rows(std::true_type{});
          else f32_rows(std::false_type{});
        }
      }
    }
    if (nxt_t < 0) break;
    cur = nxt;
    cur_t = nxt_t;
    nxt_t = __builtin_amdgcn_readfirstlane(mbox[0]);
    nxt = tile_base(nxt_t >= 0 ? nxt_t : cur_t);
    if (!early) {
      pending = sc.blk && nxt_t >= 0 && quota > 0;
      quota -= pending ? 1 : 0;
      ticket_issue_tk(wave == 0 && pending);
    }
  }
  // out of work: the run-ahead copies went into dead slots and must have landed before the stage buffers are filled again (or, at the end,
  // before the LDS belongs to someone else); steal() looks for other lists' tickets / unclaimed pairs next
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  cur_t = -1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
}  // namespace
}  // namespace alpro
