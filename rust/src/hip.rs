//! `*_hip` back-end for `cute_nucleotides` -- thin wrappers over the C ABI of
//! `libcute_nt_hip.so` (include/cute_nt.h).  Drop this file next to `n_to_bits.rs` /
//! `n_to_bits2.rs`, add `pub mod hip;` to `src/lib.rs`, and link with
//! `cargo:rustc-link-lib=dylib=cute_nt_hip` (see `build.rs`).
//!
//! NOT COMPILED in this repository's CI: the build image has no Rust toolchain.  The
//! wrappers are deliberately mechanical -- allocate a `Vec` of the exact size, call the C
//! symbol, `set_len`, return -- so that review can stand in for compilation.
//!
//! Signatures are identical to the reference's (`n_to_bits.rs:34,51`, `n_to_bits2.rs:37,78`).

use std::os::raw::{c_char, c_int, c_uint, c_void};

#[link(name = "cute_nt_hip")]
extern "C" {
    fn cnt_strerror(status: c_int) -> *const c_char;
    fn cnt_words_for(n_len: usize) -> usize;
    fn cnt_words2_for(n_len: usize) -> usize;
    fn cnt_n_to_bits_ex(n: *const u8, n_len: usize, out: *mut u64, out_words: usize, flags: c_uint) -> c_int;
    fn cnt_n_to_bits_checked(n: *const u8, n_len: usize, out: *mut u64, out_words: usize, flags: c_uint, invalid: *mut u64) -> c_int;
    fn cnt_n_to_bits2_checked(n: *const u8, n_len: usize, out: *mut u64, out_words: usize, flags: c_uint, invalid: *mut u64) -> c_int;
    fn cnt_bits_to_n(bits: *const u64, words: usize, len: usize, out: *mut u8) -> c_int;
    fn cnt_n_to_bits2(n: *const u8, n_len: usize, out: *mut u64, out_words: usize) -> c_int;
    fn cnt_n_to_bits2_ex(n: *const u8, n_len: usize, out: *mut u64, out_words: usize, flags: c_uint) -> c_int;
    fn cnt_bits_to_n2(bits: *const u64, words: usize, len: usize, out: *mut u8) -> c_int;
    fn cnt_n_to_bits_sharded(n: *const u8, n_len: usize, out: *mut u64, out_words: usize, ndev: c_int) -> c_int;
    fn cnt_bits_to_n_sharded(bits: *const u64, words: usize, len: usize, out: *mut u8, ndev: c_int) -> c_int;
    fn cnt_n_to_bits2_sharded(n: *const u8, n_len: usize, out: *mut u64, out_words: usize, ndev: c_int) -> c_int;
    fn cnt_bits_to_n2_sharded(bits: *const u64, words: usize, len: usize, out: *mut u8, ndev: c_int) -> c_int;
    // device tier (enqueue-only) + the device-memory helpers a caller without HIP bindings needs
    fn cnt_n_to_bits_dev(d_n: *const c_void, n_len: usize, d_out: *mut c_void, out_words: usize, flags: c_uint, stream: *mut c_void) -> c_int;
    fn cnt_bits_to_n_dev(d_bits: *const c_void, words: usize, len: usize, d_out: *mut c_void, flags: c_uint, stream: *mut c_void) -> c_int;
    fn cnt_n_to_bits_checked_dev(d_n: *const c_void, n_len: usize, d_out: *mut c_void, out_words: usize, flags: c_uint, d_invalid_count: *mut c_void, stream: *mut c_void) -> c_int;
    fn cnt_dev_alloc(d_ptr: *mut *mut c_void, bytes: usize) -> c_int;
    fn cnt_dev_free(d_ptr: *mut c_void) -> c_int;
    fn cnt_dev_upload(d_dst: *mut c_void, h_src: *const c_void, bytes: usize) -> c_int;
    fn cnt_dev_download(h_dst: *mut c_void, d_src: *const c_void, bytes: usize) -> c_int;
    fn cnt_dev_sync(stream: *mut c_void) -> c_int;
    fn cnt_check_device_range(p: *const c_void, bytes: usize, device: c_int) -> c_int;
    fn cnt_set_device(device: c_int) -> c_int;
    fn cnt_shutdown() -> c_int;
    // pinned caller memory: a side of a host-slice call that lies in it is used in place by the copy engines
    fn cnt_host_alloc(p: *mut *mut c_void, bytes: usize) -> c_int;
    fn cnt_host_free(p: *mut c_void) -> c_int;
    fn cnt_host_register(p: *mut c_void, bytes: usize) -> c_int;
    fn cnt_host_unregister(p: *mut c_void) -> c_int;
    fn cnt_host_is_pinned(p: *const c_void, bytes: usize) -> c_int;
    // multi-GPU device tier, enqueue-only: one library stream per shard, any number of ops queued ahead, one wait
    fn cnt_sharded_dev_open(ndev: c_int, flags: c_uint, queue: *mut *mut c_void) -> c_int;
    fn cnt_sharded_dev_open_on_streams(ndev: c_int, streams: *const *mut c_void, flags: c_uint, queue: *mut *mut c_void) -> c_int;
    fn cnt_sharded_dev_open_on_devices(ndev: c_int, devices: *const c_int, flags: c_uint, queue: *mut *mut c_void) -> c_int;
    fn cnt_sharded_dev_device(queue: *mut c_void, k: c_int, device: *mut c_int) -> c_int;
    fn cnt_sharded_dev_shards(queue: *mut c_void, ndev: *mut c_int) -> c_int;
    fn cnt_sharded_dev_wait_event(queue: *mut c_void, k: c_int, event: *mut c_void) -> c_int;
    fn cnt_sharded_dev_record_event(queue: *mut c_void, k: c_int, event: *mut c_void) -> c_int;
    fn cnt_sharded_dev_close(queue: *mut c_void) -> c_int;
    fn cnt_n_to_bits_sharded_dev_enqueue(queue: *mut c_void, d_n: *const *const c_void, n_len: *const usize, d_out: *const *mut c_void, out_words: *const usize, flags: c_uint) -> c_int;
    fn cnt_bits_to_n_sharded_dev_enqueue(queue: *mut c_void, d_bits: *const *const c_void, words: *const usize, len: *const usize, d_out: *const *mut c_void, flags: c_uint) -> c_int;
    fn cnt_n_to_bits_checked_sharded_dev_enqueue(queue: *mut c_void, d_n: *const *const c_void, n_len: *const usize, d_out: *const *mut c_void, out_words: *const usize, flags: c_uint, d_invalid_count: *const *mut c_void) -> c_int;
    fn cnt_sharded_dev_wait(queue: *mut c_void, shard_ms: *mut f32) -> c_int;
    fn cnt_sharded_dev_op_ms(queue: *mut c_void, op: usize, shard_ms: *mut f32) -> c_int;
    // packed-domain operations (host tier): what the reference's README points to, on the packed words
    fn cnt_hamming(a: *const u64, b: *const u64, len: usize, distance: *mut u64) -> c_int;
    fn cnt_complement(bits: *const u64, len: usize, out: *mut u64) -> c_int;
    fn cnt_reverse_complement(bits: *const u64, len: usize, out: *mut u64) -> c_int;
    fn cnt_validate(n: *const u8, n_len: usize, flags: c_uint, invalid: *mut u64) -> c_int;
    fn cnt_kmers_dev(d_bits: *const c_void, len: usize, k: c_uint, flags: c_uint, d_out: *mut c_void, out_cap: usize, stream: *mut c_void) -> c_int;
    fn cnt_kmers(bits: *const u64, len: usize, k: c_uint, flags: c_uint, out: *mut u64, out_cap: usize) -> c_int;
    fn cnt_kmer_counts_dev(d_bits: *const c_void, len: usize, k: c_uint, flags: c_uint, d_counts: *mut c_void, counts_cap: usize, stream: *mut c_void) -> c_int;
    fn cnt_kmer_counts(bits: *const u64, len: usize, k: c_uint, flags: c_uint, counts: *mut u64, counts_cap: usize) -> c_int;
    fn cnt_minimizers_work_bytes(len: usize, k: c_uint, w: c_uint, bytes: *mut usize) -> c_int;
    fn cnt_minimizers_dev(d_bits: *const c_void, len: usize, k: c_uint, w: c_uint, flags: c_uint, d_pos: *mut c_void, d_val: *mut c_void, out_cap: usize, d_count: *mut c_void, d_work: *mut c_void, work_bytes: usize, stream: *mut c_void) -> c_int;
    fn cnt_minimizers(bits: *const u64, len: usize, k: c_uint, w: c_uint, flags: c_uint, pos: *mut u64, val: *mut u64, out_cap: usize, count: *mut u64) -> c_int;
    fn cnt_find_pattern_work_bytes(len: usize, k: c_uint, bytes: *mut usize) -> c_int;
    fn cnt_find_pattern_dev(d_bits: *const c_void, len: usize, pattern: u64, k: c_uint, wildcards: u32, max_mismatches: c_uint, flags: c_uint, d_pos: *mut c_void, d_info: *mut c_void, out_cap: usize, d_count: *mut c_void, d_work: *mut c_void, work_bytes: usize, stream: *mut c_void) -> c_int;
    fn cnt_find_pattern(bits: *const u64, len: usize, pattern: u64, k: c_uint, wildcards: u32, max_mismatches: c_uint, flags: c_uint, pos: *mut u64, info: *mut u64, out_cap: usize, count: *mut u64) -> c_int;
    fn cnt_subseq_dev(d_bits: *const c_void, len: usize, start: usize, sub_len: usize, flags: c_uint, d_out: *mut c_void, out_words: usize, stream: *mut c_void) -> c_int;
    fn cnt_subseq(bits: *const u64, len: usize, start: usize, sub_len: usize, flags: c_uint, out: *mut u64, out_words: usize) -> c_int;
    fn cnt_extract_dev(d_bits: *const c_void, len: usize, d_start: *const c_void, d_info: *const c_void, n: usize, region_len: usize, flags: c_uint, d_out: *mut c_void, out_words: usize, d_rejected: *mut c_void, stream: *mut c_void) -> c_int;
    fn cnt_extract(bits: *const u64, len: usize, start: *const u64, info: *const u64, n: usize, region_len: usize, flags: c_uint, out: *mut u64, out_words: usize, rejected: *mut u64) -> c_int;
    fn cnt_translate_dev(d_bits: *const c_void, len: usize, start: usize, sub_len: usize, flags: c_uint, table: *const u8, d_out: *mut c_void, out_cap: usize, stream: *mut c_void) -> c_int;
    fn cnt_translate(bits: *const u64, len: usize, start: usize, sub_len: usize, flags: c_uint, table: *const u8, out: *mut u8, out_cap: usize) -> c_int;
    fn cnt_orfs_work_bytes(len: usize, bytes: *mut usize) -> c_int;
    fn cnt_orfs_dev(d_bits: *const c_void, len: usize, stops: u64, starts: u64, min_len: usize, flags: c_uint, d_pos: *mut c_void, d_length: *mut c_void, d_info: *mut c_void, out_cap: usize, d_count: *mut c_void, d_work: *mut c_void, work_bytes: usize, stream: *mut c_void) -> c_int;
    fn cnt_orfs(bits: *const u64, len: usize, stops: u64, starts: u64, min_len: usize, flags: c_uint, pos: *mut u64, length: *mut u64, info: *mut u64, out_cap: usize, count: *mut u64) -> c_int;
    fn cnt_hpc_work_bytes(len: usize, bytes: *mut usize) -> c_int;
    fn cnt_hpc_dev(d_bits: *const c_void, len: usize, flags: c_uint, d_out: *mut c_void, d_pos: *mut c_void, out_cap: usize, d_count: *mut c_void, d_work: *mut c_void, work_bytes: usize, stream: *mut c_void) -> c_int;
    fn cnt_hpc(bits: *const u64, len: usize, flags: c_uint, out: *mut u64, pos: *mut u64, out_cap: usize, count: *mut u64) -> c_int;
    fn cnt_window_counts_n(len: usize, k: c_uint, window: usize, step: usize, n_windows: *mut usize) -> c_int;
    fn cnt_window_counts_dev(d_bits: *const c_void, len: usize, k: c_uint, window: usize, step: usize, flags: c_uint, d_out: *mut c_void, out_cap: usize, stream: *mut c_void) -> c_int;
    fn cnt_window_counts(bits: *const u64, len: usize, k: c_uint, window: usize, step: usize, flags: c_uint, out: *mut u32, out_cap: usize) -> c_int;
    fn cnt_fasta_to_bits_work_bytes(text_len: usize, bytes: *mut usize) -> c_int;
    fn cnt_fasta_to_bits_dev(d_text: *const c_void, text_len: usize, flags: c_uint, d_out: *mut c_void, out_cap: usize, d_rec_text: *mut c_void, d_rec_start: *mut c_void, rec_cap: usize, d_counts: *mut c_void, d_work: *mut c_void, work_bytes: usize, stream: *mut c_void) -> c_int;
    fn cnt_fasta_to_bits(text: *const u8, text_len: usize, flags: c_uint, out: *mut u64, out_cap: usize, rec_text: *mut u64, rec_start: *mut u64, rec_cap: usize, counts: &mut [u64; 3]) -> c_int; // uint64_t counts[3]: a reference to three u64 is that pointer
    fn cnt_fastq_to_bits_work_bytes(text_len: usize, bytes: *mut usize) -> c_int;
    fn cnt_fastq_to_bits_dev(d_text: *const c_void, text_len: usize, flags: c_uint, d_out: *mut c_void, out_cap: usize, d_qual: *mut c_void, qual_cap: usize, d_rec_text: *mut c_void, d_rec_start: *mut c_void, d_rec_qual: *mut c_void, rec_cap: usize, d_counts: *mut c_void, d_work: *mut c_void, work_bytes: usize, stream: *mut c_void) -> c_int;
    fn cnt_fastq_to_bits(text: *const u8, text_len: usize, flags: c_uint, out: *mut u64, out_cap: usize, qual: *mut u8, qual_cap: usize, rec_text: *mut u64, rec_start: *mut u64, rec_qual: *mut u64, rec_cap: usize, counts: &mut [u64; 5]) -> c_int; // uint64_t counts[5]
    fn cnt_bits_to_fasta_bound(len: usize, n_rec: usize, names_len: usize, width: usize, bytes: *mut usize) -> c_int;
    fn cnt_bits_to_fasta_work_bytes(n_rec: usize, bytes: *mut usize) -> c_int;
    fn cnt_bits_to_fasta_dev(d_bits: *const c_void, len: usize, d_rec_start: *const c_void, n_rec: usize, d_names: *const c_void, names_len: usize, d_name_off: *const c_void, width: usize, flags: c_uint, d_text: *mut c_void, text_cap: usize, d_rec_text: *mut c_void, d_counts: *mut c_void, d_work: *mut c_void, work_bytes: usize, stream: *mut c_void) -> c_int;
    fn cnt_bits_to_fasta(bits: *const u64, len: usize, rec_start: *const u64, n_rec: usize, names: *const u8, names_len: usize, name_off: *const u64, width: usize, flags: c_uint, text: *mut u8, text_cap: usize, rec_text: *mut u64, counts: &mut [u64; 2]) -> c_int; // uint64_t counts[2]
    fn cnt_bits_to_fastq_bound(len: usize, n_rec: usize, names_len: usize, bytes: *mut usize) -> c_int;
    fn cnt_bits_to_fastq_work_bytes(n_rec: usize, bytes: *mut usize) -> c_int;
    fn cnt_bits_to_fastq_dev(d_bits: *const c_void, len: usize, d_qual: *const c_void, d_rec_start: *const c_void, n_rec: usize, d_names: *const c_void, names_len: usize, d_name_off: *const c_void, flags: c_uint, d_text: *mut c_void, text_cap: usize, d_rec_text: *mut c_void, d_counts: *mut c_void, d_work: *mut c_void, work_bytes: usize, stream: *mut c_void) -> c_int;
    fn cnt_bits_to_fastq(bits: *const u64, len: usize, qual: *const u8, rec_start: *const u64, n_rec: usize, names: *const u8, names_len: usize, name_off: *const u64, flags: c_uint, text: *mut u8, text_cap: usize, rec_text: *mut u64, counts: &mut [u64; 2]) -> c_int; // uint64_t counts[2]
}

const CNT_STRICT_LUT: c_uint = 1;
const CNT_TAIL_LUT: c_uint = 4;
const CNT_QUEUE_TIMED: c_uint = 1;
/// `*_checked_dev` flag: the counter is `CNT_COUNT_SLOTS` consecutive `u64` (16 KiB, zeroed by the caller) and the count is their
/// sum -- for data in which most 2-KiB tiles hold a stray (one atomic per dirty tile on ONE counter is 32 x the clean time).
pub const CNT_SPREAD_COUNT: c_uint = 8;
pub const CNT_COUNT_SLOTS: usize = 2048;

fn check(status: c_int) {
    if status != 0 {
        let msg = unsafe { std::ffi::CStr::from_ptr(cnt_strerror(status)) };
        // CNT_ELEN carries the reference's own panic text (n_to_bits.rs:53)
        panic!("{}", msg.to_string_lossy());
    }
}

/// Encode `{A, T/U, C, G}` into pairs of bits packed into 64-bit integers on the GPU.
/// Same contract as `n_to_bits_lut` (`n_to_bits.rs:34`) on the nucleotide alphabet.
pub fn n_to_bits_hip(n: &[u8]) -> Vec<u64> {
    let words = unsafe { cnt_words_for(n.len()) };
    let mut res: Vec<u64> = Vec::with_capacity(words);
    unsafe {
        check(cnt_n_to_bits_ex(n.as_ptr(), n.len(), res.as_mut_ptr(), words, 0));
        res.set_len(words);
    }
    res
}

/// As `n_to_bits_hip`, but bytes outside `ACGTUacgtu` encode as 0 like `BYTE_LUT` does.
pub fn n_to_bits_hip_strict(n: &[u8]) -> Vec<u64> {
    let words = unsafe { cnt_words_for(n.len()) };
    let mut res: Vec<u64> = Vec::with_capacity(words);
    unsafe {
        check(cnt_n_to_bits_ex(n.as_ptr(), n.len(), res.as_mut_ptr(), words, CNT_STRICT_LUT));
        res.set_len(words);
    }
    res
}

/// `n_to_bits_{pext,shift,movemask,mul}` to the letter, on ANY bytes at any length: bit extraction on whole 32-nt
/// blocks, `BYTE_LUT` on the final partial word (`n_to_bits.rs:109-111,160-162,201-203,253-255`).
pub fn n_to_bits_hip_simd_exact(n: &[u8]) -> Vec<u64> {
    let words = unsafe { cnt_words_for(n.len()) };
    let mut res: Vec<u64> = Vec::with_capacity(words);
    unsafe {
        check(cnt_n_to_bits_ex(n.as_ptr(), n.len(), res.as_mut_ptr(), words, CNT_TAIL_LUT));
        res.set_len(words);
    }
    res
}

/// `n_to_bits_hip` VALIDATED in the same pass over the data: the second value is the number of bytes of `n` outside
/// `ACGTUacgtu` -- what `BYTE_LUT` turns into code 0 without a word (`n_to_bits.rs:8-21,42`; the reference's README points at a
/// separate check, `README.md:23`).  The words are `n_to_bits_hip`'s whatever the count says.
pub fn n_to_bits_hip_checked(n: &[u8]) -> (Vec<u64>, u64) {
    let words = unsafe { cnt_words_for(n.len()) };
    let mut res: Vec<u64> = Vec::with_capacity(words);
    let mut invalid: u64 = 0;
    unsafe {
        check(cnt_n_to_bits_checked(n.as_ptr(), n.len(), res.as_mut_ptr(), words, 0, &mut invalid));
        res.set_len(words);
    }
    (res, invalid)
}

/// The validated encode as a `Result`: `Err(count)` if `n` holds `count > 0` bytes that are not nucleotides.
pub fn try_n_to_bits_hip(n: &[u8]) -> Result<Vec<u64>, u64> {
    let (res, invalid) = n_to_bits_hip_checked(n);
    if invalid == 0 {
        Ok(res)
    } else {
        Err(invalid)
    }
}

/// Decode pairs of bits from packed 64-bit integers on the GPU (`n_to_bits.rs:51`).
pub fn bits_to_n_hip(bits: &[u64], len: usize) -> Vec<u8> {
    if len > (bits.len() << 5) {
        panic!("The length is greater than the number of nucleotides!");
    }
    let mut res: Vec<u8> = Vec::with_capacity(len);
    unsafe {
        check(cnt_bits_to_n(bits.as_ptr(), bits.len(), len, res.as_mut_ptr()));
        res.set_len(len);
    }
    res
}

/// 5-letter codec (`n_to_bits2.rs:37`).
pub fn n_to_bits2_hip(n: &[u8]) -> Vec<u64> {
    let words = unsafe { cnt_words2_for(n.len()) };
    let mut res: Vec<u64> = Vec::with_capacity(words);
    unsafe {
        check(cnt_n_to_bits2(n.as_ptr(), n.len(), res.as_mut_ptr(), words));
        res.set_len(words);
    }
    res
}

/// `n_to_bits2_hip` validated in the same pass: the second value counts the bytes outside `ACGTUNacgtun` (`n_to_bits2.rs:8-23`).
pub fn n_to_bits2_hip_checked(n: &[u8]) -> (Vec<u64>, u64) {
    let words = unsafe { cnt_words2_for(n.len()) };
    let mut res: Vec<u64> = Vec::with_capacity(words);
    let mut invalid: u64 = 0;
    unsafe {
        check(cnt_n_to_bits2_checked(n.as_ptr(), n.len(), res.as_mut_ptr(), words, 0, &mut invalid));
        res.set_len(words);
    }
    (res, invalid)
}

/// `n_to_bits2_pext` to the letter on any bytes: its low-3-bit table up to word `(len - 5) / 27`, `BYTE_LUT` from there
/// on (`n_to_bits2.rs:120,179-185`).
pub fn n_to_bits2_hip_pext_exact(n: &[u8]) -> Vec<u64> {
    let words = unsafe { cnt_words2_for(n.len()) };
    let mut res: Vec<u64> = Vec::with_capacity(words);
    unsafe {
        check(cnt_n_to_bits2_ex(n.as_ptr(), n.len(), res.as_mut_ptr(), words, CNT_TAIL_LUT));
        res.set_len(words);
    }
    res
}

/// 5-letter codec (`n_to_bits2.rs:78`).
pub fn bits_to_n2_hip(bits: &[u64], len: usize) -> Vec<u8> {
    if len > bits.len() * 27 {
        panic!("The length is greater than the number of nucleotides!");
    }
    let mut res: Vec<u8> = Vec::with_capacity(len);
    unsafe {
        check(cnt_bits_to_n2(bits.as_ptr(), bits.len(), len, res.as_mut_ptr()));
        res.set_len(len);
    }
    res
}

/// `_into` forms: the same four codecs writing into a `Vec` the CALLER owns.  The `Vec` is cleared and its capacity
/// reused (grown without zero-fill when too small), so a loop that times like the reference's harness does -- the result
/// allocated AND dropped inside the timed call (`benches/bench_n_to_bits.rs:6-7`) -- pays neither the page faults of a
/// fresh allocation nor the `munmap` of the dropped one: at 1 GiB that is 22 ms per decode instead of 74 ms
/// (BENCH_r03 `host_tier`).  Same results, same panics as the returning forms.
pub fn n_to_bits_hip_into(n: &[u8], res: &mut Vec<u64>) {
    let words = unsafe { cnt_words_for(n.len()) };
    res.clear();
    res.reserve(words);
    unsafe {
        check(cnt_n_to_bits_ex(n.as_ptr(), n.len(), res.as_mut_ptr(), words, 0));
        res.set_len(words);
    }
}

pub fn bits_to_n_hip_into(bits: &[u64], len: usize, res: &mut Vec<u8>) {
    if len > (bits.len() << 5) {
        panic!("The length is greater than the number of nucleotides!");
    }
    res.clear();
    res.reserve(len);
    unsafe {
        check(cnt_bits_to_n(bits.as_ptr(), bits.len(), len, res.as_mut_ptr()));
        res.set_len(len);
    }
}

pub fn n_to_bits2_hip_into(n: &[u8], res: &mut Vec<u64>) {
    let words = unsafe { cnt_words2_for(n.len()) };
    res.clear();
    res.reserve(words);
    unsafe {
        check(cnt_n_to_bits2(n.as_ptr(), n.len(), res.as_mut_ptr(), words));
        res.set_len(words);
    }
}

pub fn bits_to_n2_hip_into(bits: &[u64], len: usize, res: &mut Vec<u8>) {
    if len > bits.len() * 27 {
        panic!("The length is greater than the number of nucleotides!");
    }
    res.clear();
    res.reserve(len);
    unsafe {
        check(cnt_bits_to_n2(bits.as_ptr(), bits.len(), len, res.as_mut_ptr()));
        res.set_len(len);
    }
}

/// Slice forms: the 2-bit codec between slices the CALLER owns -- the forms that can use PINNED memory (`PinnedBuf`, `HostPin`):
/// a side that lies in pinned memory is not staged, the copy engines read / write it in place (include/cute_nt.h "pinned caller
/// memory"; 4-10 % at 2^28 nt and above, profiles/r06_host_tier.md).  `n_to_bits_hip_slice` returns the number of words written
/// (`out` must hold `words_for(n.len())`), `bits_to_n_hip_slice` writes `len` bytes.  Same results, same panics.
pub fn n_to_bits_hip_slice(n: &[u8], out: &mut [u64]) -> usize {
    let words = unsafe { cnt_words_for(n.len()) };
    assert!(out.len() >= words);
    unsafe { check(cnt_n_to_bits_ex(n.as_ptr(), n.len(), out.as_mut_ptr(), out.len(), 0)) };
    words
}

pub fn bits_to_n_hip_slice(bits: &[u64], len: usize, out: &mut [u8]) {
    if len > (bits.len() << 5) {
        panic!("The length is greater than the number of nucleotides!");
    }
    assert!(out.len() >= len);
    unsafe { check(cnt_bits_to_n(bits.as_ptr(), bits.len(), len, out.as_mut_ptr())) };
}

/// `len` elements of pinned, device-mapped host memory (`cnt_host_alloc`), zero-filled; derefs to a slice.  For buffers that
/// live as long as the pipeline: pinned memory cannot be swapped.
pub struct PinnedBuf<T: Copy> {
    ptr: *mut T,
    len: usize,
}

impl<T: Copy> PinnedBuf<T> {
    pub fn new(len: usize) -> PinnedBuf<T> {
        let bytes = len.checked_mul(std::mem::size_of::<T>()).expect("PinnedBuf: size overflow");
        assert!(bytes > 0);
        let mut p: *mut c_void = std::ptr::null_mut();
        unsafe {
            check(cnt_host_alloc(&mut p, bytes));
            std::ptr::write_bytes(p as *mut u8, 0, bytes);
        }
        PinnedBuf { ptr: p as *mut T, len }
    }
}

impl<T: Copy> std::ops::Deref for PinnedBuf<T> {
    type Target = [T];
    fn deref(&self) -> &[T] {
        unsafe { std::slice::from_raw_parts(self.ptr, self.len) }
    }
}

impl<T: Copy> std::ops::DerefMut for PinnedBuf<T> {
    fn deref_mut(&mut self) -> &mut [T] {
        unsafe { std::slice::from_raw_parts_mut(self.ptr, self.len) }
    }
}

impl<T: Copy> Drop for PinnedBuf<T> {
    fn drop(&mut self) {
        unsafe { cnt_host_free(self.ptr as *mut c_void) };
    }
}

/// Pins an EXISTING slice in place for the guard's lifetime (`cnt_host_register`: tens of milliseconds per GiB, once;
/// unregistered on drop).  The borrow keeps the memory from being freed or moved while it is pinned.
pub struct HostPin<'a, T> {
    slice: &'a mut [T],
}

impl<'a, T> HostPin<'a, T> {
    pub fn new(slice: &'a mut [T]) -> HostPin<'a, T> {
        assert!(!slice.is_empty());
        unsafe { check(cnt_host_register(slice.as_mut_ptr() as *mut c_void, std::mem::size_of_val(slice))) };
        HostPin { slice }
    }

    pub fn get(&mut self) -> &mut [T] {
        self.slice
    }
}

impl<'a, T> Drop for HostPin<'a, T> {
    fn drop(&mut self) {
        unsafe { cnt_host_unregister(self.slice.as_mut_ptr() as *mut c_void) };
    }
}

/// Would the host tier use this slice in place?
pub fn is_pinned<T>(s: &[T]) -> bool {
    unsafe { cnt_host_is_pinned(s.as_ptr() as *const c_void, std::mem::size_of_val(s)) == 1 }
}

/// Contiguous-chunk sharding over `ndev` GPUs (0 = all visible); no collective.
pub fn n_to_bits_hip_sharded(n: &[u8], ndev: i32) -> Vec<u64> {
    let words = unsafe { cnt_words_for(n.len()) };
    let mut res: Vec<u64> = Vec::with_capacity(words);
    unsafe {
        check(cnt_n_to_bits_sharded(n.as_ptr(), n.len(), res.as_mut_ptr(), words, ndev));
        res.set_len(words);
    }
    res
}

pub fn bits_to_n_hip_sharded(bits: &[u64], len: usize, ndev: i32) -> Vec<u8> {
    if len > (bits.len() << 5) {
        panic!("The length is greater than the number of nucleotides!");
    }
    let mut res: Vec<u8> = Vec::with_capacity(len);
    unsafe {
        check(cnt_bits_to_n_sharded(bits.as_ptr(), bits.len(), len, res.as_mut_ptr(), ndev));
        res.set_len(len);
    }
    res
}

/// The 5-letter codec over `ndev` GPUs.
pub fn n_to_bits2_hip_sharded(n: &[u8], ndev: i32) -> Vec<u64> {
    let words = unsafe { cnt_words2_for(n.len()) };
    let mut res: Vec<u64> = Vec::with_capacity(words);
    unsafe {
        check(cnt_n_to_bits2_sharded(n.as_ptr(), n.len(), res.as_mut_ptr(), words, ndev));
        res.set_len(words);
    }
    res
}

pub fn bits_to_n2_hip_sharded(bits: &[u64], len: usize, ndev: i32) -> Vec<u8> {
    if len > bits.len() * 27 {
        panic!("The length is greater than the number of nucleotides!");
    }
    let mut res: Vec<u8> = Vec::with_capacity(len);
    unsafe {
        check(cnt_bits_to_n2_sharded(bits.as_ptr(), bits.len(), len, res.as_mut_ptr(), ndev));
        res.set_len(len);
    }
    res
}

// ---- operations on the packed words without decoding (README.md:20-25,45 of the reference) ----------------

fn need(bits: &[u64], len: usize) {
    if len > (bits.len() << 5) {
        panic!("The length is greater than the number of nucleotides!");
    }
}

/// Number of positions `i < len` whose 2-bit codes differ.
pub fn hamming_hip(a: &[u64], b: &[u64], len: usize) -> u64 {
    need(a, len);
    need(b, len);
    let mut d: u64 = 0;
    unsafe { check(cnt_hamming(a.as_ptr(), b.as_ptr(), len, &mut d)) };
    d
}

/// A<->T, C<->G on the packed words; unused high bits of the last word stay zero.
pub fn complement_hip(bits: &[u64], len: usize) -> Vec<u64> {
    need(bits, len);
    let words = unsafe { cnt_words_for(len) };
    let mut res: Vec<u64> = Vec::with_capacity(words);
    unsafe {
        check(cnt_complement(bits.as_ptr(), len, res.as_mut_ptr()));
        res.set_len(words);
    }
    res
}

/// `out(i) = complement(in(len - 1 - i))`.
pub fn reverse_complement_hip(bits: &[u64], len: usize) -> Vec<u64> {
    need(bits, len);
    let words = unsafe { cnt_words_for(len) };
    let mut res: Vec<u64> = Vec::with_capacity(words);
    unsafe {
        check(cnt_reverse_complement(bits.as_ptr(), len, res.as_mut_ptr()));
        res.set_len(words);
    }
    res
}

const CNT_KMER_CANONICAL: c_uint = 0x10;

/// The `len - k + 1` k-mers (`1 <= k <= 32`; none when `len < k`), each packed like a sequence of length `k`; with
/// `canonical` the smaller of the k-mer and its reverse complement as `u64` (numeric order of the packing, not letter order).
pub fn kmers_hip(bits: &[u64], len: usize, k: u32, canonical: bool) -> Vec<u64> {
    need(bits, len);
    if k == 0 || k > 32 {
        panic!("k must be in 1..32");
    }
    let m = if len >= k as usize { len - k as usize + 1 } else { 0 };
    let mut res: Vec<u64> = Vec::with_capacity(m);
    let flags = if canonical { CNT_KMER_CANONICAL } else { 0 };
    unsafe {
        check(cnt_kmers(bits.as_ptr(), len, k, flags, res.as_mut_ptr(), m));
        res.set_len(m);
    }
    res
}

/// The k-mer spectrum (`1 <= k <= 12`): `4^k` counts, entry `v` the number of k-mers whose `kmers_hip` value (same
/// `canonical`) is `v`.  `k = 1` is base composition in code order A, C, T, G.
pub fn kmer_counts_hip(bits: &[u64], len: usize, k: u32, canonical: bool) -> Vec<u64> {
    need(bits, len);
    if k == 0 || k > 12 {
        panic!("k must be in 1..12");
    }
    let bins = 1usize << (2 * k);
    let mut res: Vec<u64> = Vec::with_capacity(bins);
    let flags = if canonical { CNT_KMER_CANONICAL } else { 0 };
    unsafe {
        check(cnt_kmer_counts(bits.as_ptr(), len, k, flags, res.as_mut_ptr(), bins));
        res.set_len(bins);
    }
    res
}

/// The (w,k)-minimizers (`1 <= k <= 32`, `1 <= w <= 256`): in each window of `w` consecutive k-mers the position with the
/// smallest `(fmix64(k-mer), position)`, each distinct position once, ascending; returns the positions and their k-mers
/// (forward, or canonical as in `kmers_hip`).  No window (`len < k + w - 1`): two empty vectors.
pub fn minimizers_hip(bits: &[u64], len: usize, k: u32, w: u32, canonical: bool) -> (Vec<u64>, Vec<u64>) {
    need(bits, len);
    if k == 0 || k > 32 {
        panic!("k must be in 1..32");
    }
    if w == 0 || w > 256 {
        panic!("w must be in 1..256");
    }
    let m = if len >= k as usize { len - k as usize + 1 } else { 0 };
    let windows = if m >= w as usize { m - w as usize + 1 } else { 0 };
    // a random sequence selects about 2/(w+1) of its windows; a longer result is fetched again at its reported size
    let mut cap = std::cmp::min(windows, 2 * windows / (w as usize + 1) + windows / 16 + 64);
    let mut pos: Vec<u64> = Vec::with_capacity(cap);
    let mut val: Vec<u64> = Vec::with_capacity(cap);
    let flags = if canonical { CNT_KMER_CANONICAL } else { 0 };
    let mut n: u64 = 0;
    unsafe {
        let fits = cnt_minimizers(bits.as_ptr(), len, k, w, flags, pos.as_mut_ptr(), val.as_mut_ptr(), cap, &mut n) == 0;
        if !fits {
            // CNT_ECAP left the count in n; any other status comes back from the second call and panics in check
            cap = n as usize;
            pos = Vec::with_capacity(cap);
            val = Vec::with_capacity(cap);
            check(cnt_minimizers(bits.as_ptr(), len, k, w, flags, pos.as_mut_ptr(), val.as_mut_ptr(), cap, &mut n));
        }
        pos.set_len(n as usize);
        val.set_len(n as usize);
    }
    (pos, val)
}

/// A search pattern: `k` codes (A0 C1 T2 G3) packed like a k-mer, position j at bits 2j, and the positions that match any base.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct Pattern {
    pub pattern: u64,
    pub wildcards: u32,
    pub k: u32,
}

/// In `info` of `find_pattern_hip`: the hit is on the reverse strand.
pub const FIND_REVERSE: u64 = 0x100;
const CNT_FIND_BOTH_STRANDS: c_uint = 0x20;

/// The pattern spelled in `ACGTU` (either case) and `N` (a wildcard); `None` for any other letter or a length outside 1..32.
pub fn pattern_from_ascii(s: &[u8]) -> Option<Pattern> {
    if s.is_empty() || s.len() > 32 {
        return None;
    }
    let mut p = Pattern { pattern: 0, wildcards: 0, k: s.len() as u32 };
    for (j, ch) in s.iter().enumerate() {
        let code: u64 = match ch.to_ascii_uppercase() {
            b'A' => 0,
            b'C' => 1,
            b'T' | b'U' => 2,
            b'G' => 3,
            b'N' => {
                p.wildcards |= 1u32 << j;
                0
            }
            _ => return None,
        };
        p.pattern |= code << (2 * j);
    }
    Some(p)
}

fn find_check(p: &Pattern, max_mismatches: u32) {
    if p.k == 0 || p.k > 32 {
        panic!("k must be in 1..32");
    }
    if p.k < 32 && ((p.pattern >> (2 * p.k)) != 0 || (p.wildcards >> p.k) != 0) {
        panic!("pattern bits at or above 2k, or wildcard bits at or above k");
    }
    if max_mismatches > p.k {
        panic!("max_mismatches must be in 0..k");
    }
}

/// Where the pattern occurs with at most `max_mismatches` substitutions, on the forward strand or (`both_strands`) also where
/// the reverse strand reads it: the positions in ascending order, forward before reverse, and per hit its mismatch count plus
/// `FIND_REVERSE` on the reverse strand.  `len < k`: two empty vectors.
pub fn find_pattern_hip(bits: &[u64], len: usize, p: &Pattern, max_mismatches: u32, both_strands: bool) -> (Vec<u64>, Vec<u64>) {
    need(bits, len);
    find_check(p, max_mismatches);
    let m = if len >= p.k as usize { len - p.k as usize + 1 } else { 0 };
    let most = if both_strands { 2 * m } else { m };
    // a real search reports a handful of sites; a longer result is fetched again at its reported size
    let mut cap = std::cmp::min(most, most / 1024 + 1024);
    let mut pos: Vec<u64> = Vec::with_capacity(cap);
    let mut info: Vec<u64> = Vec::with_capacity(cap);
    let flags = if both_strands { CNT_FIND_BOTH_STRANDS } else { 0 };
    let mut n: u64 = 0;
    unsafe {
        let fits = cnt_find_pattern(bits.as_ptr(), len, p.pattern, p.k, p.wildcards, max_mismatches, flags, pos.as_mut_ptr(), info.as_mut_ptr(), cap, &mut n) == 0;
        if !fits {
            // CNT_ECAP left the count in n; any other status comes back from the second call and panics in check
            cap = n as usize;
            pos = Vec::with_capacity(cap);
            info = Vec::with_capacity(cap);
            check(cnt_find_pattern(bits.as_ptr(), len, p.pattern, p.k, p.wildcards, max_mismatches, flags, pos.as_mut_ptr(), info.as_mut_ptr(), cap, &mut n));
        }
        pos.set_len(n as usize);
        info.set_len(n as usize);
    }
    (pos, info)
}

const CNT_EXTRACT_REVCOMP: c_uint = 0x40;

fn words_of(len: usize) -> usize {
    (len >> 5) + if len & 31 != 0 { 1 } else { 0 }
}

/// Nucleotides `[start, start + sub_len)` of the sequence as a packed sequence of their own (`start` may be any nucleotide), or
/// with `revcomp` their reverse complement.  Panics when the range does not lie inside the sequence.
pub fn subseq_hip(bits: &[u64], len: usize, start: usize, sub_len: usize, revcomp: bool) -> Vec<u64> {
    need(bits, len);
    if start > len || sub_len > len - start {
        panic!("the subsequence does not lie inside the sequence");
    }
    let words = words_of(sub_len);
    let mut out: Vec<u64> = Vec::with_capacity(words);
    let flags = if revcomp { CNT_EXTRACT_REVCOMP } else { 0 };
    unsafe {
        check(cnt_subseq(bits.as_ptr(), len, start, sub_len, flags, out.as_mut_ptr(), words));
        out.set_len(words);
    }
    out
}

/// The regions `[start[i], start[i] + region_len)` of the sequence, record `i` in words `[i * R, (i + 1) * R)` of the result
/// with `R = ceil(region_len / 32)`, packed like a sequence of length `region_len`; and the number of rejected regions (those
/// that do not lie inside the sequence: their records are zero).  Region `i` is reverse-complemented iff exactly one of
/// `revcomp` and `info[i] & FIND_REVERSE` holds: `info` may be what `find_pattern_hip` returned.
pub fn extract_hip(bits: &[u64], len: usize, start: &[u64], info: Option<&[u64]>, region_len: usize, revcomp: bool) -> (Vec<u64>, u64) {
    need(bits, len);
    let n = start.len();
    let info_ptr = match info {
        Some(v) => {
            if v.len() != n {
                panic!("info must have one entry per start");
            }
            v.as_ptr()
        }
        None => std::ptr::null(),
    };
    let words = n.checked_mul(words_of(region_len)).expect("n * R overflows");
    let mut out: Vec<u64> = Vec::with_capacity(words);
    let flags = if revcomp { CNT_EXTRACT_REVCOMP } else { 0 };
    let mut rejected: u64 = 0;
    unsafe {
        check(cnt_extract(bits.as_ptr(), len, start.as_ptr(), info_ptr, n, region_len, flags, out.as_mut_ptr(), words, &mut rejected));
        out.set_len(words);
    }
    (out, rejected)
}

const CNT_TRANSLATE_REVCOMP: c_uint = 0x80;

fn table_ptr(table: Option<&[u8; 64]>) -> *const u8 {
    match table {
        Some(t) => t.as_ptr(),
        None => std::ptr::null(),
    }
}

/// Nucleotides `[start, start + sub_len)` of the sequence translated codon by codon: `sub_len / 3` bytes, one entry of `table`
/// per codon (index `x0 | x1 << 2 | x2 << 4` of the codes A0 C1 T2 G3; `None` is the standard genetic code with stops as `*`),
/// or with `revcomp` the translation of the region's reverse complement.  Forward frame `f` of a whole sequence is
/// `(f, len - f, false)`, reverse frame `f` is `(0, len - f, true)`.  Panics when the range does not lie inside the sequence.
pub fn translate_hip(bits: &[u64], len: usize, start: usize, sub_len: usize, revcomp: bool, table: Option<&[u8; 64]>) -> Vec<u8> {
    need(bits, len);
    if start > len || sub_len > len - start {
        panic!("the region does not lie inside the sequence");
    }
    let m = sub_len / 3;
    let mut out: Vec<u8> = Vec::with_capacity(m);
    let flags = if revcomp { CNT_TRANSLATE_REVCOMP } else { 0 };
    unsafe {
        check(cnt_translate(bits.as_ptr(), len, start, sub_len, flags, table_ptr(table), out.as_mut_ptr(), m));
        out.set_len(m);
    }
    out
}

const CNT_ORF_BOTH_STRANDS: c_uint = 0x200;
/// In `info` of `orfs_hip`: the ORF's opening bound is the end of the sequence, not a stop codon.
pub const ORF_OPEN_END: u64 = 0x400;
/// In `info` of `orfs_hip`: the ORF's closing bound is the end of the sequence, not a stop codon.
pub const ORF_NO_STOP: u64 = 0x800;
/// The set of the standard stop codons TAA, TGA, TAG: bit `x0 | x1 << 2 | x2 << 4` of the codes A0 C1 T2 G3.
pub const ORF_STOPS_STANDARD: u64 = (1u64 << 2) | (1u64 << 14) | (1u64 << 50);
/// The set that holds ATG alone.
pub const ORF_STARTS_ATG: u64 = 1u64 << 56;

/// The open reading frames of the sequence as `(pos, length, info)`: the stop-free runs of each frame lane, on the forward strand
/// or (`both_strands`) on both, trimmed to their first start codon (`starts == 0`: reported whole), at least `min_len`
/// nucleotides long, ordered by the upper end of the run, forward before reverse.  `stops` and `starts` are 64-bit sets of codon
/// values.  `info` is the frame plus `FIND_REVERSE`, `ORF_OPEN_END` and `ORF_NO_STOP`: `translate_hip(bits, len, pos, length,
/// reverse, None)` is the protein, and `extract_hip` takes `pos` and `info` as they are.  Panics when `stops` is empty.
pub fn orfs_hip(bits: &[u64], len: usize, stops: u64, starts: u64, min_len: usize, both_strands: bool) -> (Vec<u64>, Vec<u64>, Vec<u64>) {
    need(bits, len);
    if stops == 0 {
        panic!("stops must hold at least one codon");
    }
    let most = if len < 3 { 0 } else if both_strands { 2 * len } else { len };
    // random sequence: a stop every ~21 codons of a lane; a longer result is fetched again at its reported size
    let mut cap = std::cmp::min(most, most / 16 + 1024);
    let mut pos: Vec<u64> = Vec::with_capacity(cap);
    let mut length: Vec<u64> = Vec::with_capacity(cap);
    let mut info: Vec<u64> = Vec::with_capacity(cap);
    let flags = if both_strands { CNT_ORF_BOTH_STRANDS } else { 0 };
    let mut n: u64 = 0;
    unsafe {
        let fits = cnt_orfs(bits.as_ptr(), len, stops, starts, min_len, flags, pos.as_mut_ptr(), length.as_mut_ptr(), info.as_mut_ptr(), cap, &mut n) == 0;
        if !fits {
            // CNT_ECAP left the count in n; any other status comes back from the second call and panics in check
            cap = n as usize;
            pos = Vec::with_capacity(cap);
            length = Vec::with_capacity(cap);
            info = Vec::with_capacity(cap);
            check(cnt_orfs(bits.as_ptr(), len, stops, starts, min_len, flags, pos.as_mut_ptr(), length.as_mut_ptr(), info.as_mut_ptr(), cap, &mut n));
        }
        pos.set_len(n as usize);
        length.set_len(n as usize);
        info.set_len(n as usize);
    }
    (pos, length, info)
}

/// Homopolymer compression as `(out, n, pos)`: every run of equal bases collapses to one base.  `out` holds the `n` run bases
/// packed like any sequence (every packed-domain call takes `(&out, n)`), and `pos[j]` is where run `j` starts in the input, so
/// its length is `pos[j + 1] - pos[j]` (`len - pos[n - 1]` for the last).  `minimizers_hip(&out, n, ..)` and a look-up of its
/// positions in `pos` give the input's homopolymer-compressed minimizers.
pub fn hpc_hip(bits: &[u64], len: usize) -> (Vec<u64>, usize, Vec<u64>) {
    need(bits, len);
    // random sequence: three runs per four bases; a longer result is fetched again at its reported size
    let mut cap = std::cmp::min(len, len / 4 * 3 + len / 64 + 64);
    let mut out: Vec<u64> = vec![0u64; words_for(cap)];
    let mut pos: Vec<u64> = Vec::with_capacity(cap);
    let mut n: u64 = 0;
    unsafe {
        let fits = cnt_hpc(bits.as_ptr(), len, 0, out.as_mut_ptr(), pos.as_mut_ptr(), cap, &mut n) == 0;
        if !fits {
            // CNT_ECAP left the count in n; any other status comes back from the second call and panics in check
            cap = n as usize;
            out = vec![0u64; words_for(cap)];
            pos = Vec::with_capacity(cap);
            check(cnt_hpc(bits.as_ptr(), len, 0, out.as_mut_ptr(), pos.as_mut_ptr(), cap, &mut n));
        }
        pos.set_len(n as usize);
    }
    out.truncate(words_for(n as usize));
    (out, n as usize, pos)
}

/// FASTA text to packed words as `(out, n, rec_text, rec_start, invalid)`: header lines, line feeds and carriage returns are
/// dropped and every other byte is encoded as `n_to_bits_hip` encodes it (`strict_lut`: the byte table).  `rec_text[r]` is the
/// byte offset of header line `r`, `rec_start[r]` the position in `out` of its first base; record `r` ends where record `r + 1`
/// starts, the last one at `n`.  `invalid` counts the kept bytes outside `ACGTUacgtu` (`allow_n`: and `Nn`).
pub fn fasta_to_bits_hip(text: &[u8], strict_lut: bool, allow_n: bool) -> (Vec<u64>, usize, Vec<u64>, Vec<u64>, u64) {
    let len = text.len();
    let flags: c_uint = (if strict_lut { 1 } else { 0 }) | (if allow_n { 2 } else { 0 });
    let mut out: Vec<u64> = vec![0u64; words_for(len)];
    if len == 0 {
        return (out, 0, Vec::new(), Vec::new(), 0);
    }
    // a header every 4096 bytes or so; a longer table is fetched again at its reported size
    let mut rec_cap = std::cmp::min(len, len / 4096 + 1024);
    let mut rec_text: Vec<u64> = Vec::with_capacity(rec_cap);
    let mut rec_start: Vec<u64> = Vec::with_capacity(rec_cap);
    let mut counts = [0u64; 3];
    unsafe {
        let fits = cnt_fasta_to_bits(text.as_ptr(), len, flags, out.as_mut_ptr(), len, rec_text.as_mut_ptr(), rec_start.as_mut_ptr(), rec_cap, &mut counts) == 0;
        if !fits {
            // CNT_ECAP left the counts; any other status comes back from the second call and panics in check
            rec_cap = counts[1] as usize;
            rec_text = Vec::with_capacity(rec_cap);
            rec_start = Vec::with_capacity(rec_cap);
            check(cnt_fasta_to_bits(text.as_ptr(), len, flags, out.as_mut_ptr(), len, rec_text.as_mut_ptr(), rec_start.as_mut_ptr(), rec_cap, &mut counts));
        }
        rec_text.set_len(counts[1] as usize);
        rec_start.set_len(counts[1] as usize);
    }
    out.truncate(words_for(counts[0] as usize));
    (out, counts[0] as usize, rec_text, rec_start, counts[2])
}

/// What `fastq_to_bits_hip` returns.  Record `r` holds the bases `[rec_start[r], rec_start[r + 1])` of `out` and the qualities
/// `[rec_qual[r], rec_qual[r + 1])` of `qual`; the last record ends at `n` and at `qual.len()`.  A well-formed file has
/// `malformed == 0` and `rec_qual == rec_start`.
pub struct Fastq {
    pub out: Vec<u64>,
    pub n: usize,
    pub qual: Vec<u8>,
    pub rec_text: Vec<u64>,
    pub rec_start: Vec<u64>,
    pub rec_qual: Vec<u64>,
    pub invalid: u64,
    pub malformed: u64,
}

/// Strict four-line FASTQ text to packed words, quality bytes and a record table: a byte's role is its line number mod 4 (name,
/// sequence, separator, quality), line feeds and carriage returns are dropped, the sequence bytes are encoded as `n_to_bits_hip`
/// encodes them (`strict_lut`: the byte table), the quality bytes are copied as they are (`with_qual`).  `invalid` counts the
/// sequence bytes outside `ACGTUacgtu` (`allow_n`: and `Nn`), `malformed` the name lines without `@` plus the separators without `+`.
pub fn fastq_to_bits_hip(text: &[u8], strict_lut: bool, allow_n: bool, with_qual: bool) -> Fastq {
    let len = text.len();
    let flags: c_uint = (if strict_lut { 1 } else { 0 }) | (if allow_n { 2 } else { 0 });
    let mut out: Vec<u64> = vec![0u64; words_for(len)];
    if len == 0 {
        return Fastq { out, n: 0, qual: Vec::new(), rec_text: Vec::new(), rec_start: Vec::new(), rec_qual: Vec::new(), invalid: 0, malformed: 0 };
    }
    let mut qual: Vec<u8> = vec![0u8; if with_qual { len } else { 0 }];
    let qual_ptr = if with_qual { qual.as_mut_ptr() } else { std::ptr::null_mut() };
    // a record every 256 bytes or so; a longer table is fetched again at its reported size
    let mut rec_cap = std::cmp::min(len, len / 256 + 1024);
    let mut rec: [Vec<u64>; 3] = [Vec::with_capacity(rec_cap), Vec::with_capacity(rec_cap), Vec::with_capacity(rec_cap)];
    let mut counts = [0u64; 5];
    unsafe {
        let fits = cnt_fastq_to_bits(text.as_ptr(), len, flags, out.as_mut_ptr(), len, qual_ptr, len, rec[0].as_mut_ptr(), rec[1].as_mut_ptr(), rec[2].as_mut_ptr(), rec_cap, &mut counts) == 0;
        if !fits {
            // CNT_ECAP left the counts; any other status comes back from the second call and panics in check
            rec_cap = counts[1] as usize;
            rec = [Vec::with_capacity(rec_cap), Vec::with_capacity(rec_cap), Vec::with_capacity(rec_cap)];
            check(cnt_fastq_to_bits(text.as_ptr(), len, flags, out.as_mut_ptr(), len, qual_ptr, len, rec[0].as_mut_ptr(), rec[1].as_mut_ptr(), rec[2].as_mut_ptr(), rec_cap, &mut counts));
        }
        for r in rec.iter_mut() {
            r.set_len(counts[1] as usize);
        }
    }
    out.truncate(words_for(counts[0] as usize));
    qual.truncate(if with_qual { counts[3] as usize } else { 0 });
    let [rec_text, rec_start, rec_qual] = rec;
    Fastq { out, n: counts[0] as usize, qual, rec_text, rec_start, rec_qual, invalid: counts[2], malformed: counts[4] }
}

/// The most bytes of FASTA text `bits_to_fasta_hip` writes for `len` nucleotides in `n_rec` records whose names hold `names_len`
/// bytes, at `width` letters a line: a pure host function, the footprint of the device tier's text.
pub fn bits_to_fasta_bound(len: usize, n_rec: usize, names_len: usize, width: usize) -> usize {
    let mut bytes: usize = 0;
    unsafe { check(cnt_bits_to_fasta_bound(len, n_rec, names_len, width, &mut bytes)) };
    bytes
}

/// Packed words to FASTA text as `(text, rec_text)`: the bases in front of `rec_start[0]` as headerless lines, then per record
/// `>`, its name, a line feed and its bases `[rec_start[r], rec_start[r + 1])` -- the last record ends at `len` -- in lines of
/// `width` letters (0: one line per record).  `names` holds one name per record (or is empty: every name is empty) and is copied
/// as it is.  `rec_text[r]` is the byte offset of record `r`'s `>`.  `fasta_to_bits_hip(&text, ..)` gives `bits`, `len`,
/// `rec_start` and `rec_text` back.  Panics on a `rec_start` that descends or passes `len`; nothing is written then.
pub fn bits_to_fasta_hip(bits: &[u64], len: usize, rec_start: &[u64], names: &[&[u8]], width: usize) -> (Vec<u8>, Vec<u64>) {
    assert!(len <= bits.len() * 32, "The length is greater than the number of nucleotides!");
    let n_rec = rec_start.len();
    assert!(names.is_empty() || names.len() == n_rec, "bits_to_fasta_hip: one name per record");
    let mut name_off: Vec<u64> = Vec::with_capacity(n_rec + 1);
    let mut joined: Vec<u8> = Vec::new();
    name_off.push(0);
    for name in names {
        joined.extend_from_slice(name);
        name_off.push(joined.len() as u64);
    }
    joined.push(0); // an address even when every name is empty
    let names_len = joined.len() - 1;
    let cap = bits_to_fasta_bound(len, n_rec, names_len, width);
    let mut text: Vec<u8> = vec![0u8; std::cmp::max(cap, 1)];
    let mut rec_text: Vec<u64> = vec![0u64; n_rec];
    let mut counts = [0u64; 2];
    let (np, op) = if names.is_empty() { (std::ptr::null(), std::ptr::null()) } else { (joined.as_ptr(), name_off.as_ptr()) };
    unsafe { check(cnt_bits_to_fasta(bits.as_ptr(), len, rec_start.as_ptr(), n_rec, np, names_len, op, width, 0, text.as_mut_ptr(), cap, rec_text.as_mut_ptr(), &mut counts)) };
    text.truncate(counts[0] as usize);
    (text, rec_text)
}

/// The most bytes of FASTQ text `bits_to_fastq_hip` writes for `len` nucleotides in `n_rec` records whose names hold `names_len`
/// bytes: a pure host function, the footprint of the device tier's text.
pub fn bits_to_fastq_bound(len: usize, n_rec: usize, names_len: usize) -> usize {
    let mut bytes: usize = 0;
    unsafe { check(cnt_bits_to_fastq_bound(len, n_rec, names_len, &mut bytes)) };
    bytes
}

/// Packed words and quality bytes to four-line FASTQ text as `(text, rec_text)`: per record `@`, its name, a line feed, its bases
/// `[rec_start[r], rec_start[r + 1])` -- the first record begins at 0, the last one ends at `len` -- a line feed, `+`, a line feed,
/// the quality bytes of the same positions and a line feed.  `qual` holds `len` bytes; `names` holds one name per record (or is
/// empty: every name is empty); both are copied as they are.  `rec_text[r]` is the byte offset of record `r`'s `@`.
/// `fastq_to_bits_hip(&text, ..)` gives `bits`, `len`, `qual` and `rec_start` back.  Panics on a `rec_start` that descends, passes
/// `len` or does not begin at 0; nothing is written then.
pub fn bits_to_fastq_hip(bits: &[u64], len: usize, qual: &[u8], rec_start: &[u64], names: &[&[u8]]) -> (Vec<u8>, Vec<u64>) {
    assert!(len <= bits.len() * 32, "The length is greater than the number of nucleotides!");
    assert!(qual.len() == len, "bits_to_fastq_hip: one quality byte per nucleotide");
    let n_rec = rec_start.len();
    assert!(names.is_empty() || names.len() == n_rec, "bits_to_fastq_hip: one name per record");
    let mut name_off: Vec<u64> = Vec::with_capacity(n_rec + 1);
    let mut joined: Vec<u8> = Vec::new();
    name_off.push(0);
    for name in names {
        joined.extend_from_slice(name);
        name_off.push(joined.len() as u64);
    }
    joined.push(0); // an address even when every name is empty
    let names_len = joined.len() - 1;
    let cap = bits_to_fastq_bound(len, n_rec, names_len);
    let mut text: Vec<u8> = vec![0u8; std::cmp::max(cap, 1)];
    let mut rec_text: Vec<u64> = vec![0u64; n_rec];
    let mut counts = [0u64; 2];
    let (np, op) = if names.is_empty() { (std::ptr::null(), std::ptr::null()) } else { (joined.as_ptr(), name_off.as_ptr()) };
    unsafe { check(cnt_bits_to_fastq(bits.as_ptr(), len, qual.as_ptr(), rec_start.as_ptr(), n_rec, np, names_len, op, 0, text.as_mut_ptr(), cap, rec_text.as_mut_ptr(), &mut counts)) };
    text.truncate(counts[0] as usize);
    (text, rec_text)
}

/// The number of windows `window_counts_hip` reports: `(len - window) / step + 1`, or 0 when `len < window` (no partial window).
pub fn window_counts_n(len: usize, k: u32, window: usize, step: usize) -> usize {
    let mut n: usize = 0;
    unsafe { check(cnt_window_counts_n(len, k, window, step, &mut n)) };
    n
}

/// Base (`k = 1`) or dinucleotide (`k = 2`) counts per window: `window_counts_n` records of `4^k` counts, record `j` for the
/// positions `[j * step, j * step + window)`, entry `v` the k-mers wholly inside it whose `kmers_hip` value is `v` (`k = 1`:
/// A, C, T, G; `k = 2`: first base + 4 * second base).  `(C + G) / window` of a `k = 1` record is the window's GC content.
pub fn window_counts_hip(bits: &[u64], len: usize, k: u32, window: usize, step: usize) -> Vec<u32> {
    need(bits, len);
    let n = window_counts_n(len, k, window, step);
    let entries = n << (2 * k);
    let mut res: Vec<u32> = Vec::with_capacity(entries);
    unsafe {
        check(cnt_window_counts(bits.as_ptr(), len, k, window, step, 0, res.as_mut_ptr(), n));
        res.set_len(entries);
    }
    res
}

/// Number of bytes outside `ACGTUacgtu` (with `allow_n` also `N`/`n` are legal); 0 = a valid sequence.
pub fn validate_hip(n: &[u8], allow_n: bool) -> u64 {
    let mut bad: u64 = 0;
    unsafe { check(cnt_validate(n.as_ptr(), n.len(), if allow_n { 2 } else { 0 }, &mut bad)) };
    bad
}

// ---- device-resident tier: data already in HBM (what the roofline numbers measure) ------------------

/// Number of packed words for `n_len` nucleotides (`ceil(n_len / 32)`, n_to_bits.rs:35).
pub fn words_for(n_len: usize) -> usize {
    unsafe { cnt_words_for(n_len) }
}

/// Owned device memory on the calling thread's current device (hipMalloc / hipFree behind the C ABI).
pub struct DeviceBuffer {
    ptr: *mut c_void,
    bytes: usize,
}

impl DeviceBuffer {
    pub fn new(bytes: usize) -> DeviceBuffer {
        let mut ptr: *mut c_void = std::ptr::null_mut();
        unsafe { check(cnt_dev_alloc(&mut ptr, bytes)) };
        DeviceBuffer { ptr, bytes }
    }

    pub fn from_slice<T: Copy>(host: &[T]) -> DeviceBuffer {
        let bytes = std::mem::size_of_val(host);
        let buf = DeviceBuffer::new(bytes);
        unsafe { check(cnt_dev_upload(buf.ptr, host.as_ptr() as *const c_void, bytes)) };
        buf
    }

    /// Copies the first `len` elements back to the host (synchronous).
    pub fn to_vec<T: Copy>(&self, len: usize) -> Vec<T> {
        let bytes = len * std::mem::size_of::<T>();
        assert!(bytes <= self.bytes);
        let mut res: Vec<T> = Vec::with_capacity(len);
        unsafe {
            check(cnt_dev_download(res.as_mut_ptr() as *mut c_void, self.ptr, bytes));
            res.set_len(len);
        }
        res
    }
}

impl Drop for DeviceBuffer {
    fn drop(&mut self) {
        unsafe { cnt_dev_free(self.ptr) };
    }
}

/// Enqueue the encode of `n_len` device-resident nucleotides into `d_out` (>= `words_for(n_len)` words) on
/// the default stream; returns without waiting (`device_sync()` waits).
pub fn n_to_bits_hip_dev(d_n: &DeviceBuffer, n_len: usize, d_out: &DeviceBuffer) {
    assert!(n_len <= d_n.bytes);
    unsafe { check(cnt_n_to_bits_dev(d_n.ptr, n_len, d_out.ptr, d_out.bytes / 8, 0, std::ptr::null_mut())) };
}

/// Encode + validity count in ONE pass over the resident ASCII: the launch ADDS the number of bytes outside `ACGTUacgtu`
/// to the `u64` at the start of `d_invalid` (>= 8 bytes of device memory, zeroed by the caller).
pub fn n_to_bits_hip_checked_dev(d_n: &DeviceBuffer, n_len: usize, d_out: &DeviceBuffer, d_invalid: &DeviceBuffer) {
    assert!(n_len <= d_n.bytes && d_invalid.bytes >= 8);
    unsafe { check(cnt_n_to_bits_checked_dev(d_n.ptr, n_len, d_out.ptr, d_out.bytes / 8, 0, d_invalid.ptr, std::ptr::null_mut())) };
}

/// The same with the count spread over `CNT_COUNT_SLOTS` counters (`d_invalid`: >= 16 KiB, zeroed by the caller; the count is the
/// sum of its first `CNT_COUNT_SLOTS` words): what to use when the data is expected to be dirty.
pub fn n_to_bits_hip_checked_dev_spread(d_n: &DeviceBuffer, n_len: usize, d_out: &DeviceBuffer, d_invalid: &DeviceBuffer) {
    assert!(n_len <= d_n.bytes && d_invalid.bytes >= 8 * CNT_COUNT_SLOTS);
    unsafe { check(cnt_n_to_bits_checked_dev(d_n.ptr, n_len, d_out.ptr, d_out.bytes / 8, CNT_SPREAD_COUNT, d_invalid.ptr, std::ptr::null_mut())) };
}

/// Enqueue the decode of `len` nucleotides from `words` device-resident words into `d_out` (>= `len` bytes).
pub fn bits_to_n_hip_dev(d_bits: &DeviceBuffer, words: usize, len: usize, d_out: &DeviceBuffer) {
    if len > (words << 5) {
        panic!("The length is greater than the number of nucleotides!");
    }
    assert!(words * 8 <= d_bits.bytes && len <= d_out.bytes);
    unsafe { check(cnt_bits_to_n_dev(d_bits.ptr, words, len, d_out.ptr, 0, std::ptr::null_mut())) };
}

/// Enqueue the `len - k + 1` k-mers of `len` device-resident nucleotides into `d_out` (>= that many words); see `kmers_hip`.
pub fn kmers_hip_dev(d_bits: &DeviceBuffer, len: usize, k: u32, canonical: bool, d_out: &DeviceBuffer) {
    if len > (d_bits.bytes / 8) << 5 {
        panic!("The length is greater than the number of nucleotides!");
    }
    let flags = if canonical { CNT_KMER_CANONICAL } else { 0 };
    unsafe { check(cnt_kmers_dev(d_bits.ptr, len, k, flags, d_out.ptr, d_out.bytes / 8, std::ptr::null_mut())) };
}

/// Enqueue the k-mer spectrum of `len` device-resident nucleotides: ADDS to the `4^k` u64 counters in `d_counts` (>= that many
/// words, zeroed by the caller before the first call); see `kmer_counts_hip`.
pub fn kmer_counts_hip_dev(d_bits: &DeviceBuffer, len: usize, k: u32, canonical: bool, d_counts: &DeviceBuffer) {
    if len > (d_bits.bytes / 8) << 5 {
        panic!("The length is greater than the number of nucleotides!");
    }
    let flags = if canonical { CNT_KMER_CANONICAL } else { 0 };
    unsafe { check(cnt_kmer_counts_dev(d_bits.ptr, len, k, flags, d_counts.ptr, d_counts.bytes / 8, std::ptr::null_mut())) };
}

/// Bytes of device scratch `minimizers_hip_dev` needs for this call (0 when there is no window).
pub fn minimizers_work_bytes(len: usize, k: u32, w: u32) -> usize {
    let mut bytes: usize = 0;
    unsafe { check(cnt_minimizers_work_bytes(len, k, w, &mut bytes)) };
    bytes
}

/// Enqueue the minimizers of `len` device-resident nucleotides (see `minimizers_hip`): `d_count` (one u64) is SET to their
/// number n, the first min(n, capacity) positions go to `d_pos` and, when given, their k-mers to `d_val`; `d_work` holds at
/// least `minimizers_work_bytes` bytes of any contents.
pub fn minimizers_hip_dev(d_bits: &DeviceBuffer, len: usize, k: u32, w: u32, canonical: bool, d_pos: &DeviceBuffer, d_val: Option<&DeviceBuffer>, d_count: &DeviceBuffer, d_work: &DeviceBuffer) {
    if len > (d_bits.bytes / 8) << 5 {
        panic!("The length is greater than the number of nucleotides!");
    }
    let flags = if canonical { CNT_KMER_CANONICAL } else { 0 };
    let cap = match d_val {
        Some(v) => std::cmp::min(d_pos.bytes, v.bytes) / 8,
        None => d_pos.bytes / 8,
    };
    let val_ptr = match d_val {
        Some(v) => v.ptr,
        None => std::ptr::null_mut(),
    };
    unsafe { check(cnt_minimizers_dev(d_bits.ptr, len, k, w, flags, d_pos.ptr, val_ptr, cap, d_count.ptr, d_work.ptr, d_work.bytes, std::ptr::null_mut())) };
}

/// Bytes of device scratch `find_pattern_hip_dev` needs for this call (0 when there is no window).
pub fn find_pattern_work_bytes(len: usize, k: u32) -> usize {
    let mut bytes: usize = 0;
    unsafe { check(cnt_find_pattern_work_bytes(len, k, &mut bytes)) };
    bytes
}

/// Enqueue the search of `len` device-resident nucleotides (see `find_pattern_hip`): `d_count` (one u64) is SET to the number
/// of hits n, the first min(n, capacity) positions go to `d_pos` and, when given, their mismatch counts and strands to
/// `d_info`; `d_work` holds at least `find_pattern_work_bytes` bytes of any contents.
pub fn find_pattern_hip_dev(d_bits: &DeviceBuffer, len: usize, p: &Pattern, max_mismatches: u32, both_strands: bool, d_pos: &DeviceBuffer, d_info: Option<&DeviceBuffer>, d_count: &DeviceBuffer, d_work: &DeviceBuffer) {
    if len > (d_bits.bytes / 8) << 5 {
        panic!("The length is greater than the number of nucleotides!");
    }
    find_check(p, max_mismatches);
    let flags = if both_strands { CNT_FIND_BOTH_STRANDS } else { 0 };
    let cap = match d_info {
        Some(v) => std::cmp::min(d_pos.bytes, v.bytes) / 8,
        None => d_pos.bytes / 8,
    };
    let info_ptr = match d_info {
        Some(v) => v.ptr,
        None => std::ptr::null_mut(),
    };
    unsafe { check(cnt_find_pattern_dev(d_bits.ptr, len, p.pattern, p.k, p.wildcards, max_mismatches, flags, d_pos.ptr, info_ptr, cap, d_count.ptr, d_work.ptr, d_work.bytes, std::ptr::null_mut())) };
}

/// Enqueue the extraction of nucleotides `[start, start + sub_len)` of `len` device-resident ones into `d_out` (see
/// `subseq_hip`).
pub fn subseq_hip_dev(d_bits: &DeviceBuffer, len: usize, start: usize, sub_len: usize, revcomp: bool, d_out: &DeviceBuffer) {
    if len > (d_bits.bytes / 8) << 5 {
        panic!("The length is greater than the number of nucleotides!");
    }
    if start > len || sub_len > len - start {
        panic!("the subsequence does not lie inside the sequence");
    }
    let flags = if revcomp { CNT_EXTRACT_REVCOMP } else { 0 };
    unsafe { check(cnt_subseq_dev(d_bits.ptr, len, start, sub_len, flags, d_out.ptr, d_out.bytes / 8, std::ptr::null_mut())) };
}

/// Enqueue the extraction of the `n` regions whose starts (u64) are in `d_start` (see `extract_hip`); `d_info`, when given, holds
/// one u64 per region (what `find_pattern_hip_dev` wrote), and `d_rejected` (one u64 that the caller zeroed) has the number of
/// rejected regions ADDED to it.
pub fn extract_hip_dev(d_bits: &DeviceBuffer, len: usize, d_start: &DeviceBuffer, d_info: Option<&DeviceBuffer>, n: usize, region_len: usize, revcomp: bool, d_out: &DeviceBuffer, d_rejected: Option<&DeviceBuffer>) {
    if len > (d_bits.bytes / 8) << 5 {
        panic!("The length is greater than the number of nucleotides!");
    }
    if n > d_start.bytes / 8 {
        panic!("fewer starts than regions");
    }
    let info_ptr: *const c_void = match d_info {
        Some(v) => {
            if n > v.bytes / 8 {
                panic!("info must have one entry per start");
            }
            v.ptr as *const c_void
        }
        None => std::ptr::null(),
    };
    let rejected_ptr = match d_rejected {
        Some(v) => v.ptr,
        None => std::ptr::null_mut(),
    };
    let flags = if revcomp { CNT_EXTRACT_REVCOMP } else { 0 };
    unsafe { check(cnt_extract_dev(d_bits.ptr, len, d_start.ptr, info_ptr, n, region_len, flags, d_out.ptr, d_out.bytes / 8, rejected_ptr, std::ptr::null_mut())) };
}

/// Enqueue the translation of nucleotides `[start, start + sub_len)` of `len` device-resident ones into the `sub_len / 3` bytes of
/// `d_out` (see `translate_hip`).  `table` is host memory, read before the call returns.
pub fn translate_hip_dev(d_bits: &DeviceBuffer, len: usize, start: usize, sub_len: usize, revcomp: bool, table: Option<&[u8; 64]>, d_out: &DeviceBuffer) {
    if len > (d_bits.bytes / 8) << 5 {
        panic!("The length is greater than the number of nucleotides!");
    }
    if start > len || sub_len > len - start {
        panic!("the region does not lie inside the sequence");
    }
    let flags = if revcomp { CNT_TRANSLATE_REVCOMP } else { 0 };
    unsafe { check(cnt_translate_dev(d_bits.ptr, len, start, sub_len, flags, table_ptr(table), d_out.ptr, d_out.bytes, std::ptr::null_mut())) };
}

/// Bytes of device scratch `orfs_hip_dev` needs for a sequence of `len` nucleotides (0 below 3).
pub fn orfs_work_bytes(len: usize) -> usize {
    let mut bytes: usize = 0;
    unsafe { check(cnt_orfs_work_bytes(len, &mut bytes)) };
    bytes
}

/// Enqueue the ORF scan of `len` device-resident nucleotides (see `orfs_hip`): `d_count` (one u64) is SET to the number of
/// entries n, the first min(n, capacity) go to `d_pos`, `d_length` and, when given, `d_info`; `d_work` holds at least
/// `orfs_work_bytes` bytes of any contents.
pub fn orfs_hip_dev(d_bits: &DeviceBuffer, len: usize, stops: u64, starts: u64, min_len: usize, both_strands: bool, d_pos: &DeviceBuffer, d_length: &DeviceBuffer, d_info: Option<&DeviceBuffer>, d_count: &DeviceBuffer, d_work: &DeviceBuffer) {
    if len > (d_bits.bytes / 8) << 5 {
        panic!("The length is greater than the number of nucleotides!");
    }
    if stops == 0 {
        panic!("stops must hold at least one codon");
    }
    let flags = if both_strands { CNT_ORF_BOTH_STRANDS } else { 0 };
    let both = std::cmp::min(d_pos.bytes, d_length.bytes);
    let cap = match d_info {
        Some(v) => std::cmp::min(both, v.bytes) / 8,
        None => both / 8,
    };
    let info_ptr = match d_info {
        Some(v) => v.ptr,
        None => std::ptr::null_mut(),
    };
    unsafe { check(cnt_orfs_dev(d_bits.ptr, len, stops, starts, min_len, flags, d_pos.ptr, d_length.ptr, info_ptr, cap, d_count.ptr, d_work.ptr, d_work.bytes, std::ptr::null_mut())) };
}

/// Bytes of device scratch `hpc_hip_dev` needs for a sequence of `len` nucleotides (0 when there is none).
pub fn hpc_work_bytes(len: usize) -> usize {
    let mut bytes: usize = 0;
    unsafe { check(cnt_hpc_work_bytes(len, &mut bytes)) };
    bytes
}

/// Enqueue the homopolymer compression of `len` device-resident nucleotides (see `hpc_hip`): `d_count` (one u64) is SET to the
/// number of runs n, the first min(n, out_cap) run bases go to `d_out` packed and, when given, their positions to `d_pos`;
/// `d_out` holds at least `words_for(min(len, out_cap))` words, `d_pos` that many entries, `d_work` at least `hpc_work_bytes`
/// bytes of any contents.
pub fn hpc_hip_dev(d_bits: &DeviceBuffer, len: usize, d_out: &DeviceBuffer, d_pos: Option<&DeviceBuffer>, out_cap: usize, d_count: &DeviceBuffer, d_work: &DeviceBuffer) {
    if len > (d_bits.bytes / 8) << 5 {
        panic!("The length is greater than the number of nucleotides!");
    }
    let most = std::cmp::min(len, out_cap);
    if d_out.bytes / 8 < words_for(most) || d_pos.map_or(false, |v| v.bytes / 8 < most) {
        panic!("an output is smaller than its footprint");
    }
    let pos_ptr = match d_pos {
        Some(v) => v.ptr,
        None => std::ptr::null_mut(),
    };
    unsafe { check(cnt_hpc_dev(d_bits.ptr, len, 0, d_out.ptr, pos_ptr, out_cap, d_count.ptr, d_work.ptr, d_work.bytes, std::ptr::null_mut())) };
}

/// Bytes of device scratch `fasta_to_bits_hip_dev` needs for a text of `text_len` bytes (0 when there is none).
pub fn fasta_to_bits_work_bytes(text_len: usize) -> usize {
    let mut bytes: usize = 0;
    unsafe { check(cnt_fasta_to_bits_work_bytes(text_len, &mut bytes)) };
    bytes
}

/// Enqueue the FASTA encode of `text_len` device-resident bytes (see `fasta_to_bits_hip`): `d_counts` (three u64) is SET to `n`,
/// the number of header lines and the invalid count.  `d_out` holds at least `words_for(min(text_len, out_cap))` words, the
/// record arrays (both or neither) at least `min(text_len, rec_cap)` entries, `d_work` at least `fasta_to_bits_work_bytes` bytes.
pub fn fasta_to_bits_hip_dev(d_text: &DeviceBuffer, text_len: usize, flags: u32, d_out: &DeviceBuffer, out_cap: usize, d_rec: Option<(&DeviceBuffer, &DeviceBuffer)>, rec_cap: usize, d_counts: &DeviceBuffer, d_work: &DeviceBuffer) {
    assert!(text_len <= d_text.bytes && d_counts.bytes >= 24, "fasta_to_bits_hip_dev: sizes");
    let most = std::cmp::min(text_len, out_cap);
    let rmost = std::cmp::min(text_len, rec_cap);
    assert!(d_out.bytes / 8 >= words_for(most), "fasta_to_bits_hip_dev: out is smaller than its footprint");
    let (rt, rs) = match d_rec {
        Some((t, s)) => {
            assert!(t.bytes / 8 >= rmost && s.bytes / 8 >= rmost, "fasta_to_bits_hip_dev: a record array is smaller than its footprint");
            (t.ptr, s.ptr)
        }
        None => (std::ptr::null_mut(), std::ptr::null_mut()),
    };
    unsafe { check(cnt_fasta_to_bits_dev(d_text.ptr, text_len, flags, d_out.ptr, out_cap, rt, rs, rec_cap, d_counts.ptr, d_work.ptr, d_work.bytes, std::ptr::null_mut())) };
}

/// Bytes of device scratch `bits_to_fasta_hip_dev` needs for `n_rec` records: it depends on nothing else.
pub fn bits_to_fasta_work_bytes(n_rec: usize) -> usize {
    let mut bytes: usize = 0;
    unsafe { check(cnt_bits_to_fasta_work_bytes(n_rec, &mut bytes)) };
    bytes
}

/// Enqueue the FASTA write of `len` device-resident nucleotides (see `bits_to_fasta_hip`): `d_counts` (two u64) is SET to the bytes
/// of text and the malformed count.  `d_rec_start` holds `n_rec` entries, `d_names` (names and `n_rec + 1` offsets, or none) the
/// names back to back, `d_text` at least `min(bits_to_fasta_bound(..), text_cap)` bytes, `d_rec_text` (optional) `n_rec` entries,
/// `d_work` at least `bits_to_fasta_work_bytes(n_rec)` bytes.
pub fn bits_to_fasta_hip_dev(d_bits: &DeviceBuffer, len: usize, d_rec_start: Option<&DeviceBuffer>, n_rec: usize, d_names: Option<(&DeviceBuffer, usize, &DeviceBuffer)>, width: usize, d_text: &DeviceBuffer, text_cap: usize, d_rec_text: Option<&DeviceBuffer>, d_counts: &DeviceBuffer, d_work: &DeviceBuffer) {
    assert!(len <= (d_bits.bytes / 8) * 32 && d_counts.bytes >= 16, "bits_to_fasta_hip_dev: sizes");
    let rs = match d_rec_start {
        Some(r) => {
            assert!(r.bytes / 8 >= n_rec, "bits_to_fasta_hip_dev: rec_start is smaller than n_rec entries");
            r.ptr
        }
        None => std::ptr::null_mut(),
    };
    let (np, names_len, op) = match d_names {
        Some((n, names_len, o)) => {
            assert!(n.bytes >= names_len && o.bytes / 8 >= n_rec + 1, "bits_to_fasta_hip_dev: the name table is smaller than its extents");
            (n.ptr, names_len, o.ptr)
        }
        None => (std::ptr::null_mut(), 0, std::ptr::null_mut()),
    };
    let foot = std::cmp::min(bits_to_fasta_bound(len, n_rec, names_len, width), text_cap);
    assert!(d_text.bytes >= foot, "bits_to_fasta_hip_dev: text is smaller than its footprint");
    let rt = match d_rec_text {
        Some(r) => {
            assert!(r.bytes / 8 >= n_rec, "bits_to_fasta_hip_dev: rec_text is smaller than n_rec entries");
            r.ptr
        }
        None => std::ptr::null_mut(),
    };
    unsafe { check(cnt_bits_to_fasta_dev(d_bits.ptr, len, rs, n_rec, np, names_len, op, width, 0, d_text.ptr, text_cap, rt, d_counts.ptr, d_work.ptr, d_work.bytes, std::ptr::null_mut())) };
}

/// Bytes of device scratch `bits_to_fastq_hip_dev` needs for `n_rec` records: it depends on nothing else.
pub fn bits_to_fastq_work_bytes(n_rec: usize) -> usize {
    let mut bytes: usize = 0;
    unsafe { check(cnt_bits_to_fastq_work_bytes(n_rec, &mut bytes)) };
    bytes
}

/// Enqueue the FASTQ write of `len` device-resident nucleotides (see `bits_to_fastq_hip`): `d_counts` (two u64) is SET to the bytes
/// of text and the malformed count.  `d_qual` holds `len` bytes, `d_rec_start` `n_rec` entries, `d_names` (names and `n_rec + 1`
/// offsets, or none) the names back to back, `d_text` at least `min(bits_to_fastq_bound(..), text_cap)` bytes, `d_rec_text`
/// (optional) `n_rec` entries, `d_work` at least `bits_to_fastq_work_bytes(n_rec)` bytes.
pub fn bits_to_fastq_hip_dev(d_bits: &DeviceBuffer, len: usize, d_qual: &DeviceBuffer, d_rec_start: &DeviceBuffer, n_rec: usize, d_names: Option<(&DeviceBuffer, usize, &DeviceBuffer)>, d_text: &DeviceBuffer, text_cap: usize, d_rec_text: Option<&DeviceBuffer>, d_counts: &DeviceBuffer, d_work: &DeviceBuffer) {
    assert!(len <= (d_bits.bytes / 8) * 32 && d_qual.bytes >= len && d_rec_start.bytes / 8 >= n_rec && d_counts.bytes >= 16, "bits_to_fastq_hip_dev: sizes");
    let (np, names_len, op) = match d_names {
        Some((n, names_len, o)) => {
            assert!(n.bytes >= names_len && o.bytes / 8 >= n_rec + 1, "bits_to_fastq_hip_dev: the name table is smaller than its extents");
            (n.ptr, names_len, o.ptr)
        }
        None => (std::ptr::null_mut(), 0, std::ptr::null_mut()),
    };
    let foot = std::cmp::min(bits_to_fastq_bound(len, n_rec, names_len), text_cap);
    assert!(d_text.bytes >= foot, "bits_to_fastq_hip_dev: text is smaller than its footprint");
    let rt = match d_rec_text {
        Some(r) => {
            assert!(r.bytes / 8 >= n_rec, "bits_to_fastq_hip_dev: rec_text is smaller than n_rec entries");
            r.ptr
        }
        None => std::ptr::null_mut(),
    };
    unsafe { check(cnt_bits_to_fastq_dev(d_bits.ptr, len, d_qual.ptr, d_rec_start.ptr, n_rec, np, names_len, op, 0, d_text.ptr, text_cap, rt, d_counts.ptr, d_work.ptr, d_work.bytes, std::ptr::null_mut())) };
}

/// Bytes of device scratch `fastq_to_bits_hip_dev` needs for a text of `text_len` bytes (0 when there is none).
pub fn fastq_to_bits_work_bytes(text_len: usize) -> usize {
    let mut bytes: usize = 0;
    unsafe { check(cnt_fastq_to_bits_work_bytes(text_len, &mut bytes)) };
    bytes
}

/// Enqueue the FASTQ encode of `text_len` device-resident bytes (see `fastq_to_bits_hip`): `d_counts` (five u64) is SET to `n`, the
/// number of records, the invalid count, the number of quality bytes and the malformed count.  `d_out` holds at least
/// `words_for(min(text_len, out_cap))` words, `d_qual` (optional) at least `min(text_len, qual_cap)` bytes, the three record
/// arrays (all or none) at least `min(text_len, rec_cap)` entries, `d_work` at least `fastq_to_bits_work_bytes` bytes.
pub fn fastq_to_bits_hip_dev(d_text: &DeviceBuffer, text_len: usize, flags: u32, d_out: &DeviceBuffer, out_cap: usize, d_qual: Option<&DeviceBuffer>, qual_cap: usize, d_rec: Option<(&DeviceBuffer, &DeviceBuffer, &DeviceBuffer)>, rec_cap: usize, d_counts: &DeviceBuffer, d_work: &DeviceBuffer) {
    assert!(text_len <= d_text.bytes && d_counts.bytes >= 40, "fastq_to_bits_hip_dev: sizes");
    let most = std::cmp::min(text_len, out_cap);
    let qmost = std::cmp::min(text_len, qual_cap);
    let rmost = std::cmp::min(text_len, rec_cap);
    assert!(d_out.bytes / 8 >= words_for(most), "fastq_to_bits_hip_dev: out is smaller than its footprint");
    let qp = match d_qual {
        Some(q) => {
            assert!(q.bytes >= qmost, "fastq_to_bits_hip_dev: qual is smaller than its footprint");
            q.ptr
        }
        None => std::ptr::null_mut(),
    };
    let (rt, rs, rq) = match d_rec {
        Some((t, s, q)) => {
            assert!(t.bytes / 8 >= rmost && s.bytes / 8 >= rmost && q.bytes / 8 >= rmost, "fastq_to_bits_hip_dev: a record array is smaller than its footprint");
            (t.ptr, s.ptr, q.ptr)
        }
        None => (std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut()),
    };
    unsafe { check(cnt_fastq_to_bits_dev(d_text.ptr, text_len, flags, d_out.ptr, out_cap, qp, qual_cap, rt, rs, rq, rec_cap, d_counts.ptr, d_work.ptr, d_work.bytes, std::ptr::null_mut())) };
}

/// Enqueue the windowed counts of `len` device-resident nucleotides (see `window_counts_hip`): the `window_counts_n` records of
/// `4^k` u32 in `d_out` are SET, nothing behind them is written.  No scratch.
pub fn window_counts_hip_dev(d_bits: &DeviceBuffer, len: usize, k: u32, window: usize, step: usize, d_out: &DeviceBuffer) {
    if len > (d_bits.bytes / 8) << 5 {
        panic!("The length is greater than the number of nucleotides!");
    }
    let n = window_counts_n(len, k, window, step);
    if d_out.bytes / 4 < n << (2 * k) {
        panic!("the output is smaller than its records");
    }
    unsafe { check(cnt_window_counts_dev(d_bits.ptr, len, k, window, step, 0, d_out.ptr, n, std::ptr::null_mut())) };
}

/// Make `device` the calling thread's current device (what `DeviceBuffer::new` allocates on).
pub fn set_device(device: i32) {
    unsafe { check(cnt_set_device(device)) };
}

/// Enqueue-only multi-GPU device tier: shard `k` is resident on device `k`; every `enqueue_*` call queues that codec
/// call on every shard's own library stream and returns at once, `wait` drains all of them.  Queue the decode of step
/// `s` behind its encode and step `s + 1` behind that, wait once: the devices run back to back while the host is a
/// whole queue ahead (word `w` depends on nucleotides `[32w, 32w + 32)` only, `n_to_bits.rs:38-43`: no barrier).
pub struct ShardedDevQueue {
    handle: *mut c_void,
    ndev: usize,
}

impl ShardedDevQueue {
    /// `ndev` shards on devices `0..ndev` (`0` = all visible devices); `timed` records an event behind every op
    /// (`wait` / `op_ms` report device ms; at most 4096 ops per batch).  `self.ndev` is the shard count the LIBRARY
    /// resolved (`cnt_sharded_dev_shards`), never the caller's `0`: `wait` / `op_ms` size their buffers by it.
    pub fn new(ndev: usize, timed: bool) -> ShardedDevQueue {
        assert!(ndev <= c_int::MAX as usize);
        let mut handle: *mut c_void = std::ptr::null_mut();
        unsafe { check(cnt_sharded_dev_open(ndev as c_int, if timed { CNT_QUEUE_TIMED } else { 0 }, &mut handle)) };
        ShardedDevQueue::adopt(handle)
    }

    /// The queue adopts the caller's streams (`streams[k]`: a non-null `hipStream_t` of device `k`): shard `k`'s ops run in
    /// order with whatever else the caller enqueues there -- no host synchronisation between producer, codec and consumer.
    pub fn on_streams(streams: &[*mut c_void], timed: bool) -> ShardedDevQueue {
        assert!(!streams.is_empty() && streams.len() <= c_int::MAX as usize && streams.iter().all(|s| !s.is_null()));
        let mut handle: *mut c_void = std::ptr::null_mut();
        unsafe { check(cnt_sharded_dev_open_on_streams(streams.len() as c_int, streams.as_ptr(), if timed { CNT_QUEUE_TIMED } else { 0 }, &mut handle)) };
        ShardedDevQueue::adopt(handle)
    }

    /// Library-owned streams on an explicit device list: shard `k` runs on `devices[k]` (any subset, order or repetition of
    /// the visible devices).
    pub fn on_devices(devices: &[i32], timed: bool) -> ShardedDevQueue {
        assert!(!devices.is_empty() && devices.len() <= c_int::MAX as usize);
        let mut handle: *mut c_void = std::ptr::null_mut();
        unsafe { check(cnt_sharded_dev_open_on_devices(devices.len() as c_int, devices.as_ptr(), if timed { CNT_QUEUE_TIMED } else { 0 }, &mut handle)) };
        ShardedDevQueue::adopt(handle)
    }

    /// The device the queue runs shard `k` on -- for adopted streams what the STREAM says, not `k`.
    pub fn device(&self, k: usize) -> i32 {
        assert!(k < self.ndev);
        let mut d: c_int = -1;
        unsafe { check(cnt_sharded_dev_device(self.handle, k as c_int, &mut d)) };
        d
    }

    fn adopt(handle: *mut c_void) -> ShardedDevQueue {
        let mut n: c_int = 0;
        unsafe { check(cnt_sharded_dev_shards(handle, &mut n)) };
        assert!(n >= 1);
        ShardedDevQueue { handle, ndev: n as usize }
    }

    /// Number of shards this queue drives.
    pub fn shards(&self) -> usize {
        self.ndev
    }

    /// Shard `k`'s stream waits ON THE DEVICE for `event` (a `hipEvent_t` the caller recorded behind the work that
    /// produces shard `k`'s buffer); ops enqueued afterwards run behind it.  The host does not wait.
    pub fn wait_event(&mut self, k: usize, event: *mut c_void) {
        assert!(k < self.ndev && !event.is_null());
        unsafe { check(cnt_sharded_dev_wait_event(self.handle, k as c_int, event)) };
    }

    /// Record the caller's `hipEvent_t` (of shard `k`'s device) behind everything queued for shard `k` so far.
    pub fn record_event(&mut self, k: usize, event: *mut c_void) {
        assert!(k < self.ndev && !event.is_null());
        unsafe { check(cnt_sharded_dev_record_event(self.handle, k as c_int, event)) };
    }

    /// Queue the encode of every shard: `d_n[k]` holds `n_len[k]` nucleotides on device `k`, `d_out[k]` its words.
    pub fn enqueue_n_to_bits(&mut self, d_n: &[&DeviceBuffer], n_len: &[usize], d_out: &[&DeviceBuffer]) {
        assert!(d_n.len() == self.ndev && n_len.len() == self.ndev && d_out.len() == self.ndev);
        let ins: Vec<*const c_void> = d_n.iter().map(|b| b.ptr as *const c_void).collect();
        let outs: Vec<*mut c_void> = d_out.iter().map(|b| b.ptr).collect();
        let caps: Vec<usize> = d_out.iter().map(|b| b.bytes / 8).collect();
        for k in 0..self.ndev {
            assert!(n_len[k] <= d_n[k].bytes);
        }
        unsafe { check(cnt_n_to_bits_sharded_dev_enqueue(self.handle, ins.as_ptr(), n_len.as_ptr(), outs.as_ptr(), caps.as_ptr(), 0)) };
    }

    /// Queue the VALIDATED encode of every shard: as `enqueue_n_to_bits`, and shard `k`'s op adds the number of its bytes
    /// outside `ACGTUacgtu` to the `u64` in `d_invalid[k]` (>= 8 bytes on shard `k`'s device, zeroed by the caller).
    pub fn enqueue_n_to_bits_checked(&mut self, d_n: &[&DeviceBuffer], n_len: &[usize], d_out: &[&DeviceBuffer], d_invalid: &[&DeviceBuffer]) {
        assert!(d_n.len() == self.ndev && n_len.len() == self.ndev && d_out.len() == self.ndev && d_invalid.len() == self.ndev);
        let ins: Vec<*const c_void> = d_n.iter().map(|b| b.ptr as *const c_void).collect();
        let outs: Vec<*mut c_void> = d_out.iter().map(|b| b.ptr).collect();
        let caps: Vec<usize> = d_out.iter().map(|b| b.bytes / 8).collect();
        let counters: Vec<*mut c_void> = d_invalid.iter().map(|b| b.ptr).collect();
        for k in 0..self.ndev {
            assert!(n_len[k] <= d_n[k].bytes && d_invalid[k].bytes >= 8);
        }
        unsafe { check(cnt_n_to_bits_checked_sharded_dev_enqueue(self.handle, ins.as_ptr(), n_len.as_ptr(), outs.as_ptr(), caps.as_ptr(), 0, counters.as_ptr())) };
    }

    /// Queue the decode of every shard: `len[k]` nucleotides from `words[k]` words of `d_bits[k]` into `d_out[k]`.
    pub fn enqueue_bits_to_n(&mut self, d_bits: &[&DeviceBuffer], words: &[usize], len: &[usize], d_out: &[&DeviceBuffer]) {
        assert!(d_bits.len() == self.ndev && words.len() == self.ndev && len.len() == self.ndev && d_out.len() == self.ndev);
        for k in 0..self.ndev {
            if len[k] > (words[k] << 5) {
                panic!("The length is greater than the number of nucleotides!");
            }
            assert!(words[k] * 8 <= d_bits[k].bytes && len[k] <= d_out[k].bytes);
        }
        let ins: Vec<*const c_void> = d_bits.iter().map(|b| b.ptr as *const c_void).collect();
        let outs: Vec<*mut c_void> = d_out.iter().map(|b| b.ptr).collect();
        unsafe { check(cnt_bits_to_n_sharded_dev_enqueue(self.handle, ins.as_ptr(), words.as_ptr(), len.as_ptr(), outs.as_ptr(), 0)) };
    }

    /// Wait for everything queued; per-shard device milliseconds of the batch (zeros unless `timed`).
    pub fn wait(&mut self) -> Vec<f32> {
        let mut ms = vec![0f32; self.ndev];
        unsafe { check(cnt_sharded_dev_wait(self.handle, ms.as_mut_ptr())) };
        ms
    }

    /// Per-shard device milliseconds of op `op` of the batch the last `wait` drained (`timed` queues).
    pub fn op_ms(&self, op: usize) -> Vec<f32> {
        let mut ms = vec![0f32; self.ndev];
        unsafe { check(cnt_sharded_dev_op_ms(self.handle, op, ms.as_mut_ptr())) };
        ms
    }
}

impl Drop for ShardedDevQueue {
    fn drop(&mut self) {
        unsafe { cnt_sharded_dev_close(self.handle) };
    }
}

/// Debug aid for code that hands RAW device pointers to the `*_dev` entry points (a host pointer there is a GPU page
/// fault when the kernel runs, not an error): true if `[p, p + bytes)` lies inside one allocation the current device
/// can address.
pub fn check_device_range(p: *const c_void, bytes: usize) -> bool {
    unsafe { cnt_check_device_range(p, bytes, -1) == 0 }
}

/// Wait for everything enqueued on the default stream.
pub fn device_sync() {
    unsafe { check(cnt_dev_sync(std::ptr::null_mut())) };
}

/// Release the calling thread's cached streams / staging buffers (and the sharded tier's workers').
pub fn shutdown() {
    unsafe { check(cnt_shutdown()) };
}

#[cfg(test)]
mod tests {
    use super::*;

    // the reference's own vectors (n_to_bits.rs:412-423, n_to_bits2.rs:274-285)
    #[test]
    fn test_n_to_bits_hip() {
        assert_eq!(n_to_bits_hip(b"ATCGATCGATCGATCGATCGATCGATCGATCG"), vec![0xD8D8D8D8D8D8D8D8u64]);
        assert_eq!(n_to_bits_hip(b"ATCG"), vec![0b11011000]);
    }

    #[test]
    fn test_bits_to_n_hip() {
        assert_eq!(bits_to_n_hip(&vec![0xD8D8D8D8D8D8D8D8u64], 32), "ATCGATCGATCGATCGATCGATCGATCGATCG".as_bytes());
    }

    #[test]
    fn test_n_to_bits2_hip() {
        assert_eq!(n_to_bits2_hip(b"ATCGNATCGNATCGNATCGNATCGNATCGNATCGN"), vec![0x36A45D1F46D48BA3u64, 0x5D1F4]);
        assert_eq!(n_to_bits2_hip(b"ATCGN"), vec![0b101110100011]);
    }

    #[test]
    fn test_packed_ops() {
        let x = n_to_bits_hip(b"ATCGATCG");
        assert_eq!(hamming_hip(&x, &x, 8), 0);
        assert_eq!(hamming_hip(&x, &complement_hip(&x, 8), 8), 8);
        assert_eq!(bits_to_n_hip(&complement_hip(&x, 8), 8), b"TAGCTAGC".to_vec());
        assert_eq!(bits_to_n_hip(&reverse_complement_hip(&x, 8), 8), b"CGATCGAT".to_vec());
        assert_eq!(validate_hip(b"ACGTN", false), 1);
        assert_eq!(validate_hip(b"ACGTN", true), 0);
    }

    #[test]
    fn test_device_resident_round_trip() {
        let n = b"ATCGATCGATCGATCGATCGATCGATCGATCG";
        let d_n = DeviceBuffer::from_slice(&n[..]);
        let d_bits = DeviceBuffer::new(8);
        let d_back = DeviceBuffer::new(32);
        n_to_bits_hip_dev(&d_n, 32, &d_bits);
        bits_to_n_hip_dev(&d_bits, 1, 32, &d_back);
        device_sync();
        assert_eq!(d_bits.to_vec::<u64>(1), vec![0xD8D8D8D8D8D8D8D8u64]);
        assert_eq!(d_back.to_vec::<u8>(32), n.to_vec());
    }

    #[test]
    fn test_pinned_slices_give_the_same_words() {
        let mut n: PinnedBuf<u8> = PinnedBuf::new(1 << 22);
        for (i, b) in n.iter_mut().enumerate() {
            *b = b"ATCG"[i & 3];
        }
        assert!(is_pinned(&n[..]) && !is_pinned(&vec![0u8; 4096][..]));
        let mut out: PinnedBuf<u64> = PinnedBuf::new(words_for(n.len()));
        let words = n_to_bits_hip_slice(&n, &mut out);
        assert_eq!(words, 1 << 17);
        assert!(out.iter().all(|&w| w == 0xD8D8D8D8D8D8D8D8));
        let mut back = vec![0u8; n.len()];
        {
            let mut pin = HostPin::new(&mut back[..]);
            bits_to_n_hip_slice(&out, 1 << 22, pin.get());
        }
        assert_eq!(&back[..], &n[..]);
    }

    #[test]
    fn test_into_forms_reuse_the_callers_vec() {
        let mut words: Vec<u64> = Vec::new();
        n_to_bits_hip_into(b"ATCGATCGATCGATCGATCGATCGATCGATCG", &mut words);
        assert_eq!(words, vec![0b1101100011011000110110001101100011011000110110001101100011011000]);
        let cap = words.capacity();
        n_to_bits_hip_into(b"ATCG", &mut words);
        assert_eq!(words, vec![0b11011000]);
        assert_eq!(words.capacity(), cap);
        let mut n: Vec<u8> = Vec::new();
        bits_to_n_hip_into(&vec![0b1101100011011000110110001101100011011000110110001101100011011000], 32, &mut n);
        assert_eq!(n, b"ATCGATCGATCGATCGATCGATCGATCGATCG");
        let mut w2: Vec<u64> = Vec::new();
        n_to_bits2_hip_into(b"ATCGN", &mut w2);
        assert_eq!(w2, vec![0b101110100011]);
        bits_to_n2_hip_into(&w2, 5, &mut n);
        assert_eq!(n, b"ATCGN");
    }

    #[test]
    fn test_sharded_dev_queue_steps_ahead() {
        set_device(0);
        let n = b"ATCGATCGATCGATCGATCGATCGATCGATCG".repeat(1 << 10);
        let d_n = DeviceBuffer::from_slice(&n);
        let d_bits = DeviceBuffer::new(n.len() / 4);
        let d_back = DeviceBuffer::new(n.len());
        let mut q = ShardedDevQueue::new(1, true);
        for _ in 0..3 {
            q.enqueue_n_to_bits(&[&d_n], &[n.len()], &[&d_bits]);
            q.enqueue_bits_to_n(&[&d_bits], &[n.len() / 32], &[n.len()], &[&d_back]);
        }
        let ms = q.wait();
        assert!(ms[0] > 0.0 && q.op_ms(5)[0] > 0.0);
        assert_eq!(d_back.to_vec::<u8>(n.len()), n);
        assert!(d_bits.to_vec::<u64>(n.len() / 32).iter().all(|w| *w == 0xD8D8D8D8D8D8D8D8));
    }

    #[test]
    fn test_checked_encode_counts_what_byte_lut_zeroes() {
        assert_eq!(n_to_bits_hip_checked(b"ATCGATCG"), (vec![0xD8D8u64], 0));
        let (words, invalid) = n_to_bits_hip_checked(b"ATCGNNxx");
        assert_eq!(invalid, 4);
        assert_eq!(words, n_to_bits_hip(b"ATCGNNxx"));
        assert_eq!(try_n_to_bits_hip(b"ATCGN"), Err(1));
        assert_eq!(try_n_to_bits_hip(b"acgu"), Ok(n_to_bits_hip(b"ACGT")));
        assert_eq!(n_to_bits2_hip_checked(b"ATCGN").1, 0);
        assert_eq!(n_to_bits2_hip_checked(b"ATCGNx-").1, 2);
        let d_n = DeviceBuffer::from_slice(&b"ATCGATCGATCGATCGATCGATCGATCGAT?G"[..]);
        let d_bits = DeviceBuffer::new(8);
        let d_bad = DeviceBuffer::from_slice(&[0u64][..]);
        n_to_bits_hip_checked_dev(&d_n, 32, &d_bits, &d_bad);
        device_sync();
        assert_eq!(d_bad.to_vec::<u64>(1), vec![1u64]);
    }

    #[test]
    fn test_queue_on_an_explicit_device_list() {
        let n = b"ATCGATCGATCGATCGATCGATCGATCGATCN".repeat(64);
        let mut q = ShardedDevQueue::on_devices(&[0, 0], false);
        assert_eq!((q.shards(), q.device(0), q.device(1)), (2, 0, 0));
        set_device(0);
        let d_n = DeviceBuffer::from_slice(&n);
        let (o0, o1) = (DeviceBuffer::new(n.len() / 4), DeviceBuffer::new(n.len() / 4));
        let (c0, c1) = (DeviceBuffer::from_slice(&[0u64][..]), DeviceBuffer::from_slice(&[0u64][..]));
        q.enqueue_n_to_bits_checked(&[&d_n, &d_n], &[n.len(), n.len() - 32], &[&o0, &o1], &[&c0, &c1]);
        q.wait();
        assert_eq!((c0.to_vec::<u64>(1)[0], c1.to_vec::<u64>(1)[0]), (64, 63));
    }

    #[test]
    fn test_bits_to_n2_hip() {
        assert_eq!(bits_to_n2_hip(&vec![0x36A45D1F46D48BA3u64, 0x5D1F4], 35), "ATCGNATCGNATCGNATCGNATCGNATCGNATCGN".as_bytes());
    }
}
