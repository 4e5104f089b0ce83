// records.hip — the ownership scan of record ciphertexts: which records of a block range belong to an account (the SDK's one compute loop
// outside the prover).
//
// Replaces, for batches, what the reference runs record by record at rust/src/api/blocking.rs:213-218 and :274-276 of the reference
// (`record.is_owner_with_address_x_coordinate(&view_key, &address_x_coordinate)`, reached from RecordFinder and cli/commands/transfer.rs) and exposes as
// RecordCiphertext.isOwner (wasm/src/record/record_ciphertext.rs:63-66) — snarkVM 0.14.5 console/program/src/data/record/is_owner.rs [UPSTREAM-RECALL]:
//   private owner (a ciphertext of one field c0):  N = the prime-order point with x = nonce;  rvk = x(view_key * N);
//   randomizer = hash_many_psd8([domain "AleoSymmetricEncryption0", rvk], 1)[0];  owner <=> c0 - randomizer == address x.
// With k the odd one of {view_key, view_key + l} (l the odd subgroup order, cofactor 4), x(k (x, y)) is the same for either root y of any on-curve x:
// (x, -y) = -(x, y) + (0, -1), k (0, -1) = (0, -1) for odd k, and -(a, b) + (0, -1) = (a, -b).  Where a prime-order N with this x exists, l N = O makes the
// value x(view_key * N).  So the scan needs neither a subgroup check nor a choice of root, and is defined for every x on the curve.
//
// Here: the computation on the host (host_field.hpp, poseidon.hpp — the fallback, what small batches take, and the checker), the routing
// threshold and the one-account entry points, which take the kernel (one record per lane: records_lane.h, edwards29.h) and the device flow of the K-account scan (records_many.hip) with one key.
#include "records_strings.h"

namespace aleo_mi355x {

static int32_t records_scan(uint8_t* flags, void* rvk_out, const void* owner_c0, const void* nonce_x, size_t n, const void* view_key32, const void* address_x32, bool may_route) {
  if (!view_key32 || !address_x32 || ((!flags || !owner_c0 || !nonce_x) && n)) return bad_arg("records_scan: null buffer");
  ScanArgs a; HFr addr; if (const char* why = scan_args(a, addr, view_key32, address_x32)) return bad_arg(why);
  if (may_route && n && n >= aleo_mi355x_min_records()) {
    return scan_many_on_device(flags, rvk_out, owner_c0, nonce_x, n, ManyKeys{{a}, {addr}});
  }
  const RecordsConsts& C = records_consts();
  for (size_t i = 0; i < n; ++i)
    flags[i] = scan_one_host(rvk_out ? (uint8_t*)rvk_out + 32 * i : nullptr, (const uint8_t*)owner_c0 + 32 * i, (const uint8_t*)nonce_x + 32 * i, a, addr, C);
  return ALEO_MI355X_OK;
}

}  // namespace aleo_mi355x

using namespace aleo_mi355x;

extern "C" {

// The batch size from which a scan takes the GPU: the measured crossover against the host path on one thread, which is what a call below it runs
// (profiles/records_scan.txt: the kernel takes 2.4 ms for any batch up to 2^16; the host path 2.4 ms for 2^5 records and 4.9 ms for 2^6)
size_t aleo_mi355x_min_records(void) { return env_size("ALEO_MI355X_MIN_RECORDS", (size_t)1 << 6); }

int32_t aleo_mi355x_records_scan_host(uint8_t* flags, void* rvk_out, const void* owner_c0, const void* nonce_x, size_t n, const void* view_key32, const void* address_x32) {
  return guarded([&] { return records_scan(flags, rvk_out, owner_c0, nonce_x, n, view_key32, address_x32, false); });
}

int32_t aleo_mi355x_records_scan(uint8_t* flags, void* rvk_out, const void* owner_c0, const void* nonce_x, size_t n, const void* view_key32, const void* address_x32) {
  return guarded([&] { return records_scan(flags, rvk_out, owner_c0, nonce_x, n, view_key32, address_x32, true); });
}

}  // extern "C"
