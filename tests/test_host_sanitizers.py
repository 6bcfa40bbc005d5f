"""Host-side C++ of the product (bit packing, bincode .sketch container, FASTA / gzip readers) under
AddressSanitizer + UBSan on the CPU build: round trips, truncated files, CRLF / empty / header-only inputs."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_formats_under_asan_ubsan(tmp_path):
    exe = tmp_path / "driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "formats_sanitizer_driver.cpp"),
                           os.path.join(ROOT, "hyper-gen_amd", "csrc", "hg_formats.cpp"), "-I", os.path.join(ROOT, "include"),
                           "-lz", "-o", str(exe)])
    out = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "asan driver ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_call_pool_and_piece_packer_under_tsan(tmp_path):
    """the host threads of a host-fed call (hg_sketch_batch packs its sub-batches with them) and the hand-over between its
    uploader and its consumer under ThreadSanitizer"""
    exe = tmp_path / "pool_driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "native", "pool_tsan_driver.cpp"),
                           os.path.join(ROOT, "hyper-gen_amd", "csrc", "hg_formats.cpp"), "-I", os.path.join(ROOT, "include"),
                           "-lz", "-lpthread", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    if "FATAL: ThreadSanitizer: unexpected memory mapping" in out.stderr:
        pytest.skip("ThreadSanitizer cannot map its shadow in this container")
    assert out.returncode == 0 and "tsan driver ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_stream_chunk_layout_under_asan_ubsan(tmp_path):
    """the chunk layout of the streaming sketcher (hg_stream_layout.h: where every genome of a chunk goes, when the chunk
    closes, the size ramp, when an area grows) played through seeded push sequences of all three input kinds"""
    exe = tmp_path / "layout_driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "stream_layout_driver.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "stream layout driver ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_hostfed_batch_layout_under_asan_ubsan(tmp_path):
    """the layout of a host-fed batch (hg_hostfed_layout.h: sub-batch cuts, genome and blob offsets, which sub-batches go
    packed, upload routes, packing tasks, demotion, the decision to pack) against the loops hg_sketch_batch had before, over
    seeded length lists, and the three cases of test_hostfed_forced_packed_with_very_short_sequences"""
    exe = tmp_path / "hostfed_layout_driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "hostfed_layout_driver.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "hostfed layout driver ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_kmer_window_arithmetic_under_asan_ubsan(tmp_path):
    """the window test and the gather the amino-acid and the translated k-mer kernel share (hg_kmer_window.h, compiled
    without HIP): every k in 1..32 at every start byte 0..71 against bit-wise and byte-wise references, and the read extent
    of the kernels' largest starts inside heap blocks of the size of their LDS images"""
    exe = tmp_path / "aa_window_driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "aa_window_driver.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "aa window driver ok" in out.stdout, out.stdout + out.stderr
