"""GPU parity tests proper: the HIP path (through the C ABI) against the CPU oracle, bit-exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _dev_zeros(n):
    """Zero-filled device vector whose fill has completed: torch fills on its own stream, the library's kernels run on the
    context's (non-blocking) stream, so a pointer is only handed over once the fill is done."""
    torch = _torch()
    t = torch.zeros(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024, 2048, 4096, 8192])
def test_mdct_reverse_bit_exact(oracle, gpu_ctx, n):
    """IMdct.Reverse (Mdct.cs:13-21): HIP k_mdct_reverse == oracle restatement, every bit."""
    torch = _torch()
    rng = np.random.default_rng(n)
    batch = 37
    x = rng.uniform(-1, 1, (batch, n)).astype(np.float32)
    x[0, : n // 2] = 0.0
    x[1, : n // 2] = 1e-41  # denormals must survive
    ref = np.stack([oracle.mdct_reverse(x[b], n) for b in range(batch)])
    d = torch.from_numpy(x.copy()).cuda()
    gpu_ctx.mdct_reverse(n, batch, d.data_ptr(), n)
    gpu_ctx.synchronize()
    got = d.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), np.abs(got - ref).max()


@pytest.mark.parametrize("name", ["1test", "2test", "3test", "issue6test"])
@pytest.mark.parametrize("batch_frames", [7, 1024])
def test_ogg_files_bit_exact(oracle, gpu_ctx, ogg_bytes, name, batch_frames):
    """VorbisReader.ReadSamples over the shipped TestFiles: GPU PCM == oracle PCM, every bit."""
    import nvorbis_amd as nv
    ref, info = oracle.decode_ogg(ogg_bytes[name])
    rd = nv.VorbisReader(ogg_bytes[name], ctx=gpu_ctx, batch_frames=batch_frames)
    got = rd.read_all()
    assert rd.Channels == info["channels"]
    assert got.size == ref.size
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), np.abs(got - ref).max()
    assert rd.HasClipped == info["has_clipped"]
    rd.close()


def test_clip_samples_off(oracle, gpu_ctx, ogg_bytes):
    """IStreamDecoder.ClipSamples = false (StreamDecoder.cs:723): unclipped PCM still bit-exact."""
    import nvorbis_amd as nv
    ref, info = oracle.decode_ogg(ogg_bytes["3test"], clip=False)
    rd = nv.VorbisReader(ogg_bytes["3test"], ctx=gpu_ctx, batch_frames=100)
    rd.ClipSamples = False
    got = rd.read_all()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.abs(got).max() > 1.0  # this file really clips
    assert not rd.HasClipped
    rd.close()


def test_partial_reads(oracle, gpu_ctx, ogg_bytes):
    """ReadSamples with odd request sizes (count trimmed to a channel multiple, VorbisReader.cs:339)."""
    import nvorbis_amd as nv
    ref, info = oracle.decode_ogg(ogg_bytes["3test"])
    rd = nv.VorbisReader(ogg_bytes["3test"], ctx=gpu_ctx, batch_frames=33)
    buf = np.zeros(5001, np.float32)
    out = []
    sizes = [1, 2, 3, 999, 5001, 7, 4096]
    k = 0
    assert rd.ReadSamples(buf, 0, 1) == 0  # less than one sample frame
    while True:
        want = sizes[k % len(sizes)]
        k += 1
        n = rd.ReadSamples(buf, 0, want)
        assert n % 2 == 0 and n <= want
        if n == 0 and want >= 2:
            break
        out.append(buf[:n].copy())
    got = np.concatenate(out)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert rd.IsEndOfStream
    rd.close()


def test_fuzzed_packets_bit_exact(oracle, gpu_ctx, ogg_bytes):
    """Truncated, bit-flipped and empty packets: the reference degrades silently (SURVEY section 5, quirks
    B-14/B-16); the GPU path must produce the same PCM as the oracle for whatever survives."""
    import nvorbis_amd as nv
    rng = np.random.default_rng(77)
    for name in ("3test", "2test"):
        pk, gr, fl = nv.demux_ogg(ogg_bytes[name])
        gr, fl = gr.tolist(), fl.tolist()
        for trial in range(6):
            pk2, g2, f2 = list(pk[:3]), gr[:3], fl[:3]
            for i in range(3, len(pk)):
                p = bytearray(pk[i])
                r = rng.random()
                if r < 0.10 and len(p) > 2:
                    p = p[: int(rng.integers(0, len(p)))]
                elif r < 0.20:
                    j = int(rng.integers(0, len(p)))
                    p[j] ^= 1 << int(rng.integers(0, 8))
                elif r < 0.23:
                    p = bytearray()
                pk2.append(bytes(p))
                g2.append(gr[i])
                f2.append(fl[i])
            try:
                ref, info = oracle.decode_packets(pk2, g2, f2)
            except RuntimeError:
                with pytest.raises(nv.NvhError):
                    nv.StreamDecoder(gpu_ctx, pk2, g2, f2, 64).Read(np.zeros(1 << 22, np.float32), 0, 1 << 22)
                continue
            dec = nv.StreamDecoder(gpu_ctx, pk2, g2, f2, batch_frames=50)
            buf = np.zeros(ref.size + 4096, np.float32)
            try:
                n = dec.Read(buf, 0, buf.size - buf.size % dec.Channels)
            except nv.NvhError as e:
                # a floor curve left the dB table: the reference throws IndexOutOfRangeException; the oracle
                # reports that as an error too, so reaching this branch is a mismatch
                raise AssertionError("GPU path raised %s but the oracle decoded" % e)
            assert n == ref.size, (name, trial, n, ref.size)
            assert np.array_equal(buf[:n].view(np.uint32), ref.view(np.uint32)), (name, trial)
            dec.close()


def test_batch_repeat_and_periodicity_full_size(gpu_ctx, ogg_bytes):
    """BASELINE full size (4096 stereo long frames): repeated synthesis of a resident batch is idempotent and
    the PCM of the tiled input is periodic with the tiling period (size-independent properties)."""
    torch = _torch()
    import bench
    import nvorbis_amd as nv
    import os
    headers, ll, ch = bench.ll_packets(nv, os.path.join(bench.ROOT, "tests", "golden", "3test.ogg"))
    period = len(ll)
    st = nv.Stream(gpu_ctx, headers[0], headers[1], headers[2])
    st.push_packet(ll[0], -1, 0)
    st.synth_host()
    for i in range(4096):
        st.push_packet(ll[(i + 1) % period], -1, 0)
    b = st.upload_batch()
    assert b.frames == 4096 and b.samples == 4096 * 1024
    pcm1 = torch.zeros(b.samples * ch, dtype=torch.float32, device="cuda")
    pcm2 = torch.full_like(pcm1, 7.0)
    torch.cuda.synchronize()  # torch's fills run on its stream, the synthesis on the context's
    b.synth(pcm1.data_ptr(), pcm1.numel())
    b.synth(pcm2.data_ptr(), pcm2.numel())
    torch.cuda.synchronize()
    gpu_ctx.synchronize()
    assert torch.equal(pcm1, pcm2)
    x = pcm1.view(4096, 1024 * ch)
    # frame f and frame f+period have identical packets and identical predecessors (f >= 1)
    assert torch.equal(x[1:4096 - period], x[1 + period:4096])
    assert bool(torch.isfinite(pcm1).all()) and float(pcm1.abs().max()) <= 0.99999994 + 1e-9
    b.free()
    st.close()


@pytest.mark.parametrize("workload", ["greal", "c3_markov", "grand_mono_tail"])
def test_resident_batches_vs_oracle(oracle, gpu_ctx, ogg_bytes, workload):
    """The path bench.py times -- packets parsed once, the batch resident in HBM (nvh_batch_upload), synthesised by the slab
    kernels with paired emission (even frames overlap-add, clip and interleave in k_synth; k_ola_compact only over the frames
    outside the steady state) -- against the oracle, bit for bit: the bench workload, a 256 / 2048 Markov stream on full-depth
    packets (block-size switches inside the batch), and batches cut at odd / even lengths so that the last frame is an emitter
    once and a plane writer once.  Synthesised twice into different buffers (resident means repeatable)."""
    torch = _torch()
    import bench
    import nvorbis_amd as nv
    import os
    from tests import vorbis_encode as ve
    if workload == "greal":
        headers, ll, ch = bench.ll_packets(nv, os.path.join(bench.ROOT, "tests", "golden", "3test.ogg"))
        audio = [ll[i % len(ll)] for i in range(701)]
        cuts = [700]
    else:
        hdr3 = ve.shipped_headers(ogg_bytes["3test"])
        S3 = ve.setup_of(hdr3)
        pool3 = ve.packet_pool(S3, 20260928, per_kind=64)
        kinds = ve.markov_kinds(np.random.default_rng(11), 1300) if workload == "c3_markov" else np.ones(1300, dtype=bool)
        p, _ = ve.stream_from_pool(S3, hdr3, pool3, kinds, np.random.default_rng(5))
        headers, audio, ch = p[:3], p[3:], 2
        cuts = [1200] if workload == "c3_markov" else [511, 512]
    packets = list(headers) + list(audio)
    ref, info = oracle.decode_packets(packets, [-1] * len(packets), [0] * len(packets))
    for cut in cuts:
        st = nv.Stream(gpu_ctx, headers[0], headers[1], headers[2])
        st.push_packet(audio[0], -1, 0)
        first = st.synth_host()  # the first packet primes the overlap and emits nothing (StreamDecoder.cs:446-450)
        assert first.size == 0
        for i in range(cut):
            st.push_packet(audio[1 + i], -1, 0)
        b = st.upload_batch()
        assert b.frames == cut
        n = b.samples * ch
        pcm1 = torch.zeros(n, dtype=torch.float32, device="cuda")
        pcm2 = torch.full_like(pcm1, 7.0)
        torch.cuda.synchronize()
        b.synth(pcm1.data_ptr(), n)
        b.synth(pcm2.data_ptr(), n)
        gpu_ctx.synchronize()
        torch.cuda.synchronize()
        got = pcm1.cpu().numpy()
        assert n <= ref.size
        assert np.array_equal(got.view(np.uint32), ref[:n].view(np.uint32)), (workload, cut, float(np.abs(got - ref[:n]).max()))
        assert torch.equal(pcm1, pcm2)
        b.free()
        st.close()


def test_bench_workload_prefix_vs_oracle(oracle, gpu_ctx):
    """First 600 frames of the bench workload against the oracle, bit-exact."""
    import bench
    import nvorbis_amd as nv
    import os
    headers, ll, ch = bench.ll_packets(nv, os.path.join(bench.ROOT, "tests", "golden", "3test.ogg"))
    packets = list(headers) + [ll[i % len(ll)] for i in range(601)]
    ref, info = oracle.decode_packets(packets, [-1] * len(packets), [0] * len(packets))
    dec = nv.StreamDecoder(gpu_ctx, packets, batch_frames=256)
    buf = np.zeros(ref.size + 64, np.float32)
    n = dec.Read(buf, 0, buf.size)
    # 600 overlapped frames + the drained tail of the last one when the provider runs dry (StreamDecoder.cs:352-356)
    assert n == ref.size == (600 * 1024 + 1024) * ch
    assert np.array_equal(buf[:n].view(np.uint32), ref.view(np.uint32))
    dec.close()


def _decode_gpu(nv, ctx, pk, gr, fl, clip, batch_frames):
    dec = nv.StreamDecoder(ctx, pk, gr, fl, batch_frames=batch_frames)
    dec.ClipSamples = clip
    chunks = []
    buf = np.zeros(1 << 20, np.float32)
    buf = buf[: buf.size - buf.size % dec.Channels]
    while True:
        n = dec.Read(buf, 0, buf.size)
        if n == 0:
            break
        chunks.append(buf[:n].copy())
    dec.close()
    return np.concatenate(chunks) if chunks else np.zeros(0, np.float32)


@pytest.mark.parametrize("name", ["mono_res0_small_blocks", "stereo_res1_coupled", "three_ch_res2_misaligned", "six_ch_res2_4096",
                                  "two_submaps", "equal_blocks_overrun", "mono_8192", "stereo_8192", "mono_res1_2048", "floor0_slab",
                                  "ch9_res2", "ch16_res1_4096", "ch40_res1"])
@pytest.mark.parametrize("consistent", [True, False])
def test_synthetic_configs_bit_exact(oracle, gpu_ctx, name, consistent):
    """Paths no shipped file reaches -- Residue0, Residue1 with coupling, 3 and 6 channels (incl. the Residue2
    offset quirk B-1 and BASELINE config C4's shape), several submaps (quirk B-3), block sizes 64/128 and 8192,
    codebook dimensions that do not divide the partition size, inconsistent window flags (sequential overlap
    path), 9 / 16 / 40 channels (the descriptor kernels and k_ola_compact's scalar loop; execute flags of channels
    32 and beyond) -- bit-exact against the oracle on random-bit packets."""
    import nvorbis_amd as nv
    from tests import synth_stream as ss
    pk, gr, fl = ss.filtered_stream(oracle, name, 150, 11 + int(consistent), consistent_windows=consistent)
    for clip in (True, False):
        ref, info = oracle.decode_packets(pk, gr, fl, clip=clip)
        for bf in (1024, 13):
            got = _decode_gpu(nv, gpu_ctx, pk, gr, fl, clip, bf)
            assert got.size == ref.size, (name, clip, bf)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (name, clip, bf, float(np.abs(got - ref).max()))


@pytest.mark.parametrize("name", ["res0_slab", "odd_dims_slab", "res2_alias_stereo", "two_pass_slab", "res0_3ch"])
@pytest.mark.parametrize("consistent", [True, False])
def test_general_bin_walk_bit_exact(oracle, gpu_ctx, name, consistent):
    """The slab kernels' general bin walk (kernels_synth.hip: residue_walk_general; host_slab.cpp: residue_general): Residue0,
    lattice books of dimension 1 / 3 / 5, Residue2 over two channels whose 15-component partitions share bins (quirk B-1), two
    residue passes per frame (Mapping.cs:122-134 calls every submap's residue over every channel).  Bit-exact against the
    oracle, and -- on the default path -- synthesised by k_synth_g / k_synth8_g (k_synth / k_synth8 + the general walk) rather than the descriptor kernels."""
    import os
    import nvorbis_amd as nv
    from tests import synth_stream as ss
    pk, gr, fl = ss.filtered_stream(oracle, name, 150, 31 + int(consistent), consistent_windows=consistent)
    for clip in (True, False):
        ref, info = oracle.decode_packets(pk, gr, fl, clip=clip)
        for bf in (1024, 13):
            got = _decode_gpu(nv, gpu_ctx, pk, gr, fl, clip, bf)
            assert got.size == ref.size, (name, clip, bf)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (name, clip, bf, float(np.abs(got - ref).max()))
    toggles = ("NVH_UNFUSED", "NVH_NO_FUSED_IMDCT", "NVH_NO_COMPACT", "NVH_NO_SLAB")
    if consistent and not any(os.environ.get(t) for t in toggles):
        torch = _torch()
        # ... with the packets parsed on the host, and with the GPU packet parser writing the group lists itself (round 5)
        for gpu_parse in (False, True):
            st = nv.Stream(gpu_ctx, pk[0], pk[1], pk[2])
            if gpu_parse:
                st.set_gpu_parse(True)
            for p in pk[3:40]:
                st.push_packet(p, -1, 0)
            b = st.upload_batch()
            pcm = torch.empty(max(b.samples * st.channels, 1), dtype=torch.float32, device="cuda")
            b.synth(pcm.data_ptr(), pcm.numel())
            names = [k for k in b.kernels() if k != "-"]
            b.free(); st.close()
            kn = "k_synth8_g" if name == "res0_3ch" else "k_synth_g"
            assert names and kn in names and all(k in (kn, "k_ola_compact", "k_parse_slab", "k_parse_links") for k in names), (gpu_parse, names)


@pytest.mark.parametrize("name", ["table_books_pair", "table_books_general", "table_books_b1"])
@pytest.mark.parametrize("consistent", [True, False])
def test_table_books_take_the_slab_kernels(oracle, gpu_ctx, name, consistent):
    """Books with an explicit table -- lookup type 2 and type 1 with sequence_p (Codebook.cs:262-281) -- in residues of the slab
    kernels' shapes: a slab record names such a book by lat_values = 0 and the walks gather the component from the VQ pool
    (kernels_synth.hip: table_value; round 6 -- through round 5 these streams took the descriptor kernels).  The pair walk, the
    general bin walk and the quirk-B-1 bin walk, host-parsed and GPU-parsed: bit-exact against the oracle, and synthesised by
    the slab kernels on the default path."""
    import os
    import nvorbis_amd as nv
    from tests import synth_stream as ss
    pk, gr, fl = ss.filtered_stream(oracle, name, 150, 41 + int(consistent), consistent_windows=consistent)
    for clip in (True, False):
        ref, info = oracle.decode_packets(pk, gr, fl, clip=clip)
        for bf in (1024, 13):
            got = _decode_gpu(nv, gpu_ctx, pk, gr, fl, clip, bf)
            assert got.size == ref.size, (name, clip, bf)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (name, clip, bf, float(np.abs(got - ref).max()))
    toggles = ("NVH_UNFUSED", "NVH_NO_FUSED_IMDCT", "NVH_NO_COMPACT", "NVH_NO_SLAB")
    if consistent and not any(os.environ.get(t) for t in toggles):
        torch = _torch()
        for gpu_parse in (False, True):
            st = nv.Stream(gpu_ctx, pk[0], pk[1], pk[2])
            if gpu_parse:
                st.set_gpu_parse(True)
            for p in pk[3:40]:
                st.push_packet(p, -1, 0)
            b = st.upload_batch()
            pcm = torch.empty(max(b.samples * st.channels, 1), dtype=torch.float32, device="cuda")
            b.synth(pcm.data_ptr(), pcm.numel())
            names = [k for k in b.kernels() if k != "-"]
            b.free(); st.close()
            assert names and all(k.startswith("k_synth") or k in ("k_ola_compact", "k_parse_slab", "k_parse_links") for k in names), (gpu_parse, names)
            if name == "table_books_general":
                assert "k_synth_g" in names, (gpu_parse, names)


def test_vector_overrun_takes_the_general_walk(oracle, gpu_ctx):
    """Book dimensions that do not divide the partition size (Residue1.cs:12-22, Residue2.cs:27-45: whole entries are added, the
    last one runs over into the next partition's elements): the general bin walk merges the two partitions that touch a bin anyway
    and takes the spill as part of the earlier partition's vector write (round 6; kernels_synth.hip: residue_walk_general, `span`;
    through round 5: the descriptor kernels).  Bit-exact against the oracle (test_synthetic_configs_bit_exact has the long form);
    here: the kernels that ran, for both parsers."""
    import os
    import nvorbis_amd as nv
    from tests import synth_stream as ss
    if any(os.environ.get(t) for t in ("NVH_UNFUSED", "NVH_NO_FUSED_IMDCT", "NVH_NO_COMPACT", "NVH_NO_SLAB")):
        pytest.skip("a replay that forces the descriptor kernels")
    torch = _torch()
    pk, gr, fl = ss.filtered_stream(oracle, "equal_blocks_overrun", 120, 17)
    ref, info = oracle.decode_packets(pk, gr, fl, clip=True)
    for gpu_parse in (False, True):
        st = nv.Stream(gpu_ctx, pk[0], pk[1], pk[2])
        if gpu_parse:
            st.set_gpu_parse(True)
        for i in range(3, len(pk)):
            st.push_packet(pk[i], int(gr[i]), int(fl[i]))
        st.push_end()
        b = st.upload_batch()
        pcm = torch.empty(max(b.samples * st.channels, 1), dtype=torch.float32, device="cuda")
        b.synth(pcm.data_ptr(), pcm.numel())
        gpu_ctx.synchronize()
        names = [k for k in b.kernels() if k != "-"]
        got = pcm.cpu().numpy()[:b.samples * st.channels]
        b.free(); st.close()
        assert "k_synth_g" in names and all(k in ("k_synth_g", "k_ola_compact", "k_parse_slab", "k_parse_links") for k in names), (gpu_parse, names)
        assert got.size == ref.size and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), gpu_parse


@pytest.mark.parametrize("name", ["ch4_res1", "ch5_res2", "ch7_res1", "ch8_res2"])
def test_channel_counts_4_5_7_8_bit_exact(oracle, gpu_ctx, name):
    """Every channel count has its own instantiation of the overlap-add kernels (ola_vec / ola_sym_lds<CH>) and of the
    eight-channel synthesis kernel's coupling and floor loops; 1, 2, 3 and 6 channels come with the configs above, these
    are the other four (k_synth8 by default; the descriptor kernels in the NVH_NO_SLAB replay below)."""
    import nvorbis_amd as nv
    from tests import synth_stream as ss
    pk, gr, fl = ss.filtered_stream(oracle, name, 120, 23)
    for clip in (True, False):
        ref, info = oracle.decode_packets(pk, gr, fl, clip=clip)
        for bf in (1024, 13):
            got = _decode_gpu(nv, gpu_ctx, pk, gr, fl, clip, bf)
            assert got.size == ref.size, (name, clip, bf)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (name, clip, bf, float(np.abs(got - ref).max()))


_KERNEL_TOGGLES = ("NVH_EMIT_ALWAYS", "NVH_UNFUSED", "NVH_NO_FUSED_IMDCT", "NVH_NO_COMPACT", "NVH_GPU_PARSE", "NVH_COPY_UPLOAD",
                   "NVH_NO_EMIT", "NVH_NO_EMIT8", "NVH_NO_SLAB", "NVH_POISON_PLANES")


@pytest.mark.parametrize("name", ["ch9_res2", "ch16_res1_4096", "ch40_res1"])
def test_wide_configs_take_the_descriptor_kernels(oracle, gpu_ctx, name):
    """More than eight channels are outside the slab contract (NVH_SLAB_MAX_CH) and the GPU parser's: the descriptor kernels
    and k_ola_compact's scalar loop (kernels.hip) decode them.  Sixteen channels at n = 4096 (128 KiB of spectra, a
    residue with vector overrun: no 152 KB LDS window) take the global-memory pair k_residue + k_couple_floor, nine and forty
    channels the LDS-resident k_spectrum_gen8.  Bit-exact against the oracle on the structured stream of tests/spec_pin.py,
    whose silent channels include channels beyond 31."""
    import os
    import nvorbis_amd as nv
    from tests import spec_pin
    torch = _torch()
    pk, gr = (list(x) for x in spec_pin.stream(name))
    fl = [0] * len(pk)
    ref, _ = oracle.decode_packets(pk, gr, fl, clip=False)
    for bf in (1024, 5):
        got = _decode_gpu(nv, gpu_ctx, pk, gr, fl, False, bf)
        assert got.size == ref.size and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (bf, float(np.abs(got - ref).max()))
    st = nv.Stream(gpu_ctx, pk[0], pk[1], pk[2])
    for p in pk[3:]:
        st.push_packet(p, -1, 0)
    b = st.upload_batch()
    pcm = torch.empty(max(b.samples * st.channels, 1), dtype=torch.float32, device="cuda")
    b.synth(pcm.data_ptr(), pcm.numel())
    names = [k for k in b.kernels() if k != "-"]
    b.free()
    st.close()
    assert not any(k.startswith("k_synth") for k in names), names
    if not any(os.environ.get(t) for t in _KERNEL_TOGGLES):
        assert "k_ola_compact" in names, names
        if name == "ch16_res1_4096":
            assert "k_residue" in names and "k_couple_floor" in names, names
        else:
            assert "k_spectrum_gen8" in names, names


@pytest.mark.parametrize("name", ["ch9_res2", "ch16_res1_4096", "ch40_res1"])
def test_gpu_parser_refuses_wide_streams(oracle, gpu_ctx, name):
    """The GPU packet parser takes at most NVH_PARSE_MAX_CH channels: set_gpu_parse raises ERR_UNSUPPORTED (as for Floor0), and
    VorbisReader(gpu_parse=True) -- whose StreamDecoder asks for it -- keeps the host parser and returns the oracle's PCM."""
    import nvorbis_amd as nv
    from nvorbis_amd import native
    from tests import ogg_py, spec_pin
    pk, gr = (list(x) for x in spec_pin.stream(name))
    st = nv.Stream(gpu_ctx, pk[0], pk[1], pk[2])
    try:
        with pytest.raises(native.NvhError) as e:
            st.set_gpu_parse(True)
        assert e.value.code == native.ERR_UNSUPPORTED
    finally:
        st.close()
    data = ogg_py.write_ogg(pk, gr)
    ref, info = oracle.decode_ogg(data, clip=False)
    rd = nv.VorbisReader(data, ctx=gpu_ctx, batch_frames=7, gpu_parse=True)
    rd.ClipSamples = False
    got = rd.read_all()
    assert rd.Channels == info["channels"]
    rd.close()
    assert got.size == ref.size > 0
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("name", ["stereo_res1_coupled", "three_ch_res2_misaligned", "six_ch_res2_4096", "floor0_stereo", "floor0_slab",
                                  "two_submaps", "equal_blocks_overrun", "mono_8192", "stereo_8192", "ch4_res1", "ch5_res2", "ch7_res1",
                                  "ch8_res2", "mono_res1_2048", "res0_slab", "odd_dims_slab", "res2_alias_stereo", "two_pass_slab",
                                  "res0_3ch", "table_books_pair", "table_books_general", "table_books_b1", "ch9_res2", "ch16_res1_4096",
                                  "ch40_res1"])
def test_gpu_matches_the_spec_decoder(gpu_ctx, name):
    """The product's PCM (clip off) on every pinned configuration's structured stream against the spec-derived decoder with the
    configuration's quirk set (tests/spec_pin.py), within the CPU pin's bound (1e-6 x peak; Floor0 spec_pin.FLOOR0_BOUND): no
    oracle in between.  In the replays that force the descriptor kernels this is the high-precision check of k_spectrum_f0's
    device cos / sqrt / exp.  The spec decode is cached per process (spec_pin.spec_pcm)."""
    import nvorbis_amd as nv
    from tests import spec_pin
    pk, gr = (list(x) for x in spec_pin.stream(name))
    want = spec_pin.spec_pcm(name, tuple(sorted(spec_pin.QUIRKS[name])))
    got = _decode_gpu(nv, gpu_ctx, pk, gr, [0] * len(pk), False, 1024).astype(np.float64)
    assert got.size == want.size
    peak = float(np.abs(want).max())
    assert float(np.abs(got - want).max()) <= spec_pin.bound(name) * peak, (name, float(np.abs(got - want).max()) / peak)


def test_floor0_within_tolerance(oracle, gpu_ctx):
    """Floor0 evaluates cos / sqrt / exp in double precision (Floor0.cs:167,198,201).  On the default path the host parser's
    thread evaluates the curve's value per Bark section with the same libm the oracle uses (host_slab.cpp:
    floor0_section_values) and the kernel only gathers and multiplies: bit-exact by construction.  The descriptor kernels
    (k_spectrum_f0: the replays of this suite with NVH_UNFUSED / NVH_NO_FUSED_IMDCT / NVH_NO_COMPACT / NVH_NO_SLAB) use the device
    math library, for which nothing guarantees the last bit of a double: the north star's 1e-6 is what is asserted there."""
    import os
    import nvorbis_amd as nv
    from tests import synth_stream as ss
    for name in ("floor0_stereo", "floor0_slab"):  # (odd-dimension books: descriptor kernels; lattice books: the slab kernels)
        pk, gr, fl = ss.filtered_stream(oracle, name, 200, 5)
        ref, info = oracle.decode_packets(pk, gr, fl, clip=True)
        got = _decode_gpu(nv, gpu_ctx, pk, gr, fl, True, 64)
        assert got.size == ref.size
        assert np.isfinite(got).all()
        assert float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()) <= 1e-6
        exact = float((got.view(np.uint32) == ref.view(np.uint32)).mean())
        # Both configurations take the slab kernels by default (floor0_stereo's odd-dimension books through the general bin walk
        # since round 4), where Floor0 is host-evaluated: bit-exact.  Only the replays that force the descriptor kernels
        # (k_spectrum_f0: device cos / sqrt / exp) are held to the tolerance alone.
        if not any(os.environ.get(t) for t in ("NVH_UNFUSED", "NVH_NO_FUSED_IMDCT", "NVH_NO_COMPACT", "NVH_NO_SLAB")):
            assert exact == 1.0, (name, exact)
        else:
            assert exact > 0.99, (name, exact)


@pytest.mark.parametrize("toggle", ["NVH_EMIT_ALWAYS", "NVH_UNFUSED", "NVH_NO_FUSED_IMDCT", "NVH_NO_COMPACT", "NVH_GPU_PARSE",
                                    "NVH_EMIT_ALWAYS+NVH_GPU_PARSE", "NVH_COPY_UPLOAD+NVH_GPU_PARSE", "NVH_NO_EMIT", "NVH_NO_EMIT8", "NVH_NO_SLAB",
                                    "NVH_POISON_PLANES", "NVH_POISON_PLANES+NVH_GPU_PARSE", "NVH_FPW=1", "NVH_FPW=4",
                                    "NVH_FPW=1+NVH_GPU_PARSE", "NVH_FPW=4+NVH_GPU_PARSE", "NVH_FPW=4+NVH_POISON_PLANES"])
def test_fallback_kernel_paths_bit_exact(toggle):
    """The library picks kernel variants by stream shape.  The default path of every stream the slab
    kernels take is host-written (or GPU-parsed) slabs -> k_synth / k_synth8 with paired emission; each environment toggle
    switches one level of that off or an opt-in on, and the whole parity suite above is replayed that way in a child process:
    NVH_EMIT_ALWAYS -> paired emission (k_synth_emit; k_synth8_emit for wide frames) for every batch with a steady-state frame,
    not only those that are 7/8 steady state; NVH_NO_EMIT -> the slab kernels without paired emission (every overlap-add in
    k_ola_compact), NVH_NO_EMIT8 -> the same for wide frames only; NVH_NO_SLAB -> the descriptor kernels (k_spectrum_imdct & co.) that serve the shapes outside the
    slab contract -- these three replays take tests/test_full_depth.py (C2 / C3 / C4 / C5 on full-depth packets) along;
    NVH_UNFUSED -> k_residue + k_couple_floor, NVH_NO_FUSED_IMDCT -> k_spectrum + k_imdct_compact, NVH_NO_COMPACT -> k_imdct_wave +
    k_ola_emit; NVH_GPU_PARSE -> packets parsed on the GPU (k_parse_slab writes the slabs; k_parse's descriptors for the shapes outside the slab
    contract) instead of by the host parser; NVH_COPY_UPLOAD -> its input goes up by copy commands instead of k_parse_fetch;
    NVH_POISON_PLANES -> every batch's work planes start out as NaN bit patterns (hipMemsetAsync at upload): device blocks are
    recycled through a pool and never cleared, so a kernel that read a plane region nothing wrote in this batch would get by on
    what an earlier decode left there -- the replay turns that into NaN PCM (round 5: the library has no such read; what
    round 4 saw with planes in hipDeviceMallocUncached memory was the platform, tools/ubench/uncached_handoff.hip);
    NVH_FPW=1 -> paired emission with one frame per workgroup (k_synth + k_synth_emit, k_synth_tail when a batch's last decoded
    frame is odd) instead of the default frame groups of two (k_synth_group2), NVH_FPW=4 -> frame groups of four (k_synth_group4;
    k_synth + k_synth_emit for batches whose slabs leave no room for four frames' LDS) -- these two replays take
    tests/test_full_depth.py and tests/test_frame_groups.py along.  A part KEY=VALUE sets KEY to VALUE, a bare KEY sets it to 1."""
    import os
    import subprocess
    import sys
    if os.environ.get("NVH_TEST_CHILD"):
        pytest.skip("already inside a fallback-path run")
    env = dict(os.environ)
    for t in toggle.split("+"):  # "A+B": both switches (slab kernels fed by the GPU packet parser)
        key, _, val = t.partition("=")
        env[key] = val or "1"
    env["NVH_TEST_CHILD"] = "1"
    from tests.replay import run_children
    children = [(["test_gpu_parity.py"], env, [])]
    if toggle in ("NVH_EMIT_ALWAYS", "NVH_NO_EMIT", "NVH_NO_EMIT8", "NVH_NO_SLAB"):
        children.append((["test_full_depth.py"], env, []))  # (a second child beside the first)
    if toggle in ("NVH_FPW=1", "NVH_FPW=4"):
        children.append((["test_full_depth.py"], env, []))  # (three children beside this process: four with the GPU open)
        children.append((["test_frame_groups.py"], env, []))
    run_children(children, timeout=900)


def _level1_in_mapping_order(oracle, gpu_ctx, pk, pick):
    """Mode.Decode of single packets assembled from the level-1 entry points, called in the order Mapping.DecodePacket and
    Mode.Decode call the plug-in interfaces (Mapping.cs:95-198, Mode.cs:153-170):
        Array.Clear -> IResidue.Decode per submap -> inverse coupling, last step first -> per channel IFloor.Apply +
        IMdct.Reverse (or clearing the back half) -> window loop
    -- what csharp/GpuFactory.cs's classes do -- must equal nvh_mode_decode of the same packet, bit for bit.  The bit-consuming
    results each call needs (posts / LSP coefficients, execute flags, the packet cursor at every IResidue.Decode) are the
    oracle's for that packet."""
    import ctypes as C
    import nvorbis_amd as nv
    torch = _torch()
    L = oracle.L
    d = oracle.open_headers(pk[:3])
    st = nv.Stream(gpu_ctx, pk[0], pk[1], pk[2])
    checked = 0
    try:
        ch, b1 = st.channels, st.block1
        nmodes = L.orc_mode_info(d, 0, None, None, None)
        mode_bits = max(0, (nmodes - 1).bit_length())
        ref_planes = np.zeros(ch * b1, np.float32)
        want = _dev_zeros(ch * b1)
        for i in pick:
            p = pk[i]
            a, b, c, e = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            rc = L.orc_decode_packet_block(d, p, len(p), ref_planes.ctypes.data, C.byref(a), C.byref(b), C.byref(c), C.byref(e))
            geo = st.mode_decode(p, want.data_ptr())
            if rc != 1 or geo is None:
                continue
            n = e.value
            bits = int.from_bytes(p[:8].ljust(8, b"\0"), "little")
            mode_idx = (bits >> 1) & ((1 << mode_bits) - 1)
            flag, bs, mp = C.c_int(), C.c_int(), C.c_int()
            L.orc_mode_info(d, mode_idx, C.byref(flag), C.byref(bs), C.byref(mp))
            assert bs.value == n
            prev_f = (bits >> (1 + mode_bits)) & 1 if flag.value else 0
            next_f = (bits >> (2 + mode_bits)) & 1 if flag.value else 0
            steps = C.c_int()
            mag, ang, chfl = np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(16, np.int32)
            assert L.orc_mapping_info(d, mp.value, C.byref(steps), mag.ctypes.data, ang.ctypes.data, 64, chfl.ctypes.data, 16) == 0
            # IFloorData of every channel
            ex, posts, counts, amps, coeffs, ftype = [], [], [], [], [], []
            for cc in range(ch):
                xe, pc, am = C.c_int(), C.c_int(), C.c_float()
                po, co = np.zeros(64, np.int32), np.zeros(257, np.float32)
                t = L.orc_last_floor_data(d, cc, C.byref(xe), po.ctypes.data, C.byref(pc), C.byref(am), co.ctypes.data, 257)
                assert t >= 0
                ex.append(bool(xe.value)); posts.append(po); counts.append(pc.value); amps.append(am.value); coeffs.append(co); ftype.append(t)
            # buffers as DecodeNextPacket hands them over: whatever the previous packet left, front halves cleared (Mapping.cs:108)
            host = np.random.default_rng(i).normal(0, 1, ch * b1).astype(np.float32).reshape(ch, b1)
            host[:, : n // 2] = 0.0
            planes = torch.from_numpy(host.reshape(-1).copy()).cuda()
            torch.cuda.synchronize()
            base = planes.data_ptr()
            pos, idx, any_ = np.zeros(16, np.int32), np.zeros(16, np.int32), C.c_int()
            ncalls = L.orc_last_residue_calls(d, pos.ctypes.data, idx.ctypes.data, 16, C.byref(any_))
            for k in range(ncalls):  # IResidue.Decode per submap (Mapping.cs:122-134)
                st.residue_decode(int(idx[k]), p, int(pos[k]), n, base, any_channel_decodes=bool(any_.value))
            for k in range(steps.value - 1, -1, -1):  # inverse coupling (Mapping.cs:137-182)
                if ex[int(ang[k])] or ex[int(mag[k])]:
                    gpu_ctx.inverse_couple(base + 4 * b1 * int(mag[k]), base + 4 * b1 * int(ang[k]), n // 2)
            for cc in range(ch):  # IFloor.Apply + IMdct.Reverse (Mapping.cs:185-197)
                row = base + 4 * b1 * cc
                if ex[cc]:
                    if ftype[cc] == 1:
                        status = st.floor1_apply(int(chfl[cc]), n, posts[cc].reshape(1, 64), np.array([counts[cc]], np.int32), row, b1)
                    else:
                        am = amps[cc]
                        status = st.floor0_apply(int(chfl[cc]), n, np.array([am], np.float32), coeffs[cc][:256].reshape(1, 256), row, b1)
                    assert status[0] == 0
                    gpu_ctx.mdct_reverse(n, 1, row, b1)
                else:
                    gpu_ctx.synchronize()
                    planes.view(ch, b1)[cc, n // 2:n] = 0.0  # Array.Clear(buffer[c], halfBlockSize, halfBlockSize)
                    torch.cuda.synchronize()
            st.window_apply(mode_idx, prev_f, next_f, ch, base, b1)  # Mode.cs:160-166
            gpu_ctx.synchronize()
            got = planes.cpu().numpy().reshape(ch, b1)[:, :n]
            exp = want.cpu().numpy().reshape(ch, b1)[:, :n]
            if any(t == 0 for t in ftype):
                assert float(np.abs(got - exp).max()) <= 1e-6
            else:
                assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (i, float(np.abs(got - exp).max()))
            checked += 1
    finally:
        st.close()
        L.orc_close(d)
    return checked


@pytest.mark.parametrize("name", ["2test", "3test"])
def test_level1_entries_in_mapping_order_files(oracle, gpu_ctx, ogg_bytes, name):
    import nvorbis_amd as nv
    pk, gr, fl = nv.demux_ogg(ogg_bytes[name])
    pick = list(range(3, 30)) + list(range(30, len(pk), max(1, (len(pk) - 30) // 40)))
    assert _level1_in_mapping_order(oracle, gpu_ctx, pk, pick) >= 40


@pytest.mark.parametrize("name", ["stereo_res1_coupled", "three_ch_res2_misaligned", "six_ch_res2_4096", "two_submaps", "mono_res0_small_blocks"])
def test_level1_entries_in_mapping_order_synthetic(oracle, gpu_ctx, name):
    from tests import synth_stream as ss
    pk, gr, fl = ss.filtered_stream(oracle, name, 40, 3)
    assert _level1_in_mapping_order(oracle, gpu_ctx, pk, range(3, len(pk))) >= 20


def test_level1_entries_in_mapping_order_c4_full_depth(oracle, gpu_ctx, ogg_bytes):
    from tests import vorbis_encode as ve
    hdr = ve.c4_headers(ve.shipped_headers(ogg_bytes["3test"]), psize=32)
    S = ve.setup_of(hdr)
    kinds = np.ones(10, dtype=bool)
    kinds[4:6] = False
    pk, gr = ve.encode_stream(S, hdr, kinds, 9)
    assert _level1_in_mapping_order(oracle, gpu_ctx, pk, range(3, len(pk))) == 10


def test_six_channel_four_wavefront_kernel_bit_exact():
    """Streams with more than four channels run k_spectrum_gen8 (8 wavefronts per workgroup); NVH_NO_GEN8 sends them
    through k_spectrum_gen instead: the six-channel cases replayed in a child process."""
    import os
    import subprocess
    import sys
    if os.environ.get("NVH_TEST_CHILD"):
        pytest.skip("already inside a fallback-path run")
    env = dict(os.environ)
    env["NVH_NO_GEN8"] = "1"
    env["NVH_TEST_CHILD"] = "1"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_parity.py"), "-x", "-q", "-m", "gpu",
                        "-k", "six_ch", "-p", "no:cacheprovider"], cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]


def test_threaded_corpus_decode_matches_serial(oracle, ogg_bytes):
    """File-parallel decode with a pool of host threads on one GPU (corpus.decode_files_threaded) returns, per file,
    exactly the oracle's PCM: concurrent contexts / HIP streams do not interfere."""
    from nvorbis_amd import corpus
    names = ["1test", "2test", "3test", "issue6test"] * 3
    files = [ogg_bytes[n] for n in names]
    out = corpus.decode_files_threaded(files, device=0, workers=6, batch_frames=512)
    refs = {n: oracle.decode_ogg(ogg_bytes[n])[0] for n in set(names)}
    for n, o in zip(names, out):
        assert o.size == refs[n].size and (o == refs[n]).all(), n


def test_inverse_couple_bit_exact(oracle, gpu_ctx):
    """Fine-grained ABI: one inverse coupling step (Mapping.cs:150-178) on device vectors == the oracle's, every bit."""
    import ctypes as C
    torch = _torch()
    rng = np.random.default_rng(5)
    n = 4099
    m = rng.normal(0, 1, n).astype(np.float32)
    a = rng.normal(0, 1, n).astype(np.float32)
    m[:8] = [0.0, -0.0, 1.0, -1.0, 0.0, 1e-41, -1e-41, 3.0]
    a[:8] = [0.0, 1.0, 0.0, -0.0, -2.0, 1e-41, 1e-41, -3.0]
    rm, ra = m.copy(), a.copy()
    oracle.L.orc_inverse_couple(rm.ctypes.data, ra.ctypes.data, n)
    dm, da = torch.from_numpy(m.copy()).cuda(), torch.from_numpy(a.copy()).cuda()
    gpu_ctx.inverse_couple(dm.data_ptr(), da.data_ptr(), n)
    gpu_ctx.synchronize()
    assert np.array_equal(dm.cpu().numpy().view(np.uint32), rm.view(np.uint32))
    assert np.array_equal(da.cpu().numpy().view(np.uint32), ra.view(np.uint32))


@pytest.mark.parametrize("name", ["2test", "3test"])
def test_mode_decode_blocks_bit_exact(oracle, gpu_ctx, ogg_bytes, name):
    """Fine-grained ABI: IMode.Decode of single packets (windowed blocks before overlap, Mode.cs:153-170) == the oracle's
    orc_decode_packet_block, for long, short and transition windows."""
    import ctypes as C
    import nvorbis_amd as nv
    torch = _torch()
    pk, gr, fl = nv.demux_ogg(ogg_bytes[name])
    hdr = pk[:3]
    blob = np.frombuffer(b"".join(hdr), dtype=np.uint8)
    offs = np.zeros(4, np.int64)
    offs[1:] = np.cumsum([len(p) for p in hdr])
    g3, f3, err = np.full(3, -1, np.int64), np.zeros(3, np.uint8), C.c_int(0)
    d = oracle.L.orc_open_packets(blob.ctypes.data, offs.ctypes.data, g3.ctypes.data, f3.ctypes.data, 3, C.byref(err))
    assert d
    st = nv.Stream(gpu_ctx, pk[0], pk[1], pk[2])
    try:
        ch, b1 = st.channels, st.block1
        ref = np.zeros(ch * b1, np.float32)
        got = _dev_zeros(ch * b1)
        kinds = set()
        step = max(1, (len(pk) - 3) // 60)
        for i in list(range(3, min(len(pk), 40))) + list(range(40, len(pk), step)):
            a, b, c, e = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            rc = oracle.L.orc_decode_packet_block(d, pk[i], len(pk[i]), ref.ctypes.data, C.byref(a), C.byref(b), C.byref(c), C.byref(e))
            geo = st.mode_decode(pk[i], got.data_ptr())
            assert (rc == 1) == (geo is not None), i
            if geo is None:
                continue
            assert geo == (e.value, a.value, b.value, c.value), (i, geo)
            n = e.value
            kinds.add((n, a.value, c.value))
            g = got.cpu().numpy().reshape(ch, b1)[:, :n]
            r = ref.reshape(ch, b1)[:, :n]
            assert np.array_equal(g.view(np.uint32), r.view(np.uint32)), (i, float(np.abs(g - r).max()))
        assert len(kinds) >= 2  # more than one window shape was exercised
    finally:
        st.close()
        oracle.L.orc_close(d)


@pytest.mark.parametrize("name", ["mono_res0_small_blocks", "stereo_res1_coupled", "three_ch_res2_misaligned", "six_ch_res2_4096",
                                  "two_submaps", "equal_blocks_overrun", "mono_8192", "floor0_stereo"])
def test_mode_decode_synthetic_shapes(oracle, gpu_ctx, name):
    """IMode.Decode per packet for the stream shapes no shipped file has (Residue0/1, 3 and 6 channels, submaps, 64..8192
    blocks): bit-exact, Floor0 within the stated 1e-6."""
    import ctypes as C
    import nvorbis_amd as nv
    from tests import synth_stream as ss
    torch = _torch()
    pk, gr, fl = ss.filtered_stream(oracle, name, 40, 21)
    hdr = pk[:3]
    blob = np.frombuffer(b"".join(hdr), dtype=np.uint8)
    offs = np.zeros(4, np.int64)
    offs[1:] = np.cumsum([len(p) for p in hdr])
    g3, f3, err = np.full(3, -1, np.int64), np.zeros(3, np.uint8), C.c_int(0)
    d = oracle.L.orc_open_packets(blob.ctypes.data, offs.ctypes.data, g3.ctypes.data, f3.ctypes.data, 3, C.byref(err))
    assert d
    st = nv.Stream(gpu_ctx, pk[0], pk[1], pk[2])
    try:
        ch, b1 = st.channels, st.block1
        ref = np.zeros(ch * b1, np.float32)
        got = _dev_zeros(ch * b1)
        seen = 0
        for i in range(3, len(pk)):
            a, b, c, e = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            rc = oracle.L.orc_decode_packet_block(d, pk[i], len(pk[i]), ref.ctypes.data, C.byref(a), C.byref(b), C.byref(c), C.byref(e))
            geo = st.mode_decode(pk[i], got.data_ptr())
            assert (rc == 1) == (geo is not None), i
            if geo is None:
                continue
            seen += 1
            n = e.value
            g = got.cpu().numpy().reshape(ch, b1)[:, :n]
            r = ref.reshape(ch, b1)[:, :n]
            if name == "floor0_stereo":
                assert float(np.abs(g.astype(np.float64) - r.astype(np.float64)).max()) <= 1e-6, i
            else:
                assert np.array_equal(g.view(np.uint32), r.view(np.uint32)), (i, float(np.abs(g - r).max()))
        assert seen > 10
    finally:
        st.close()
        oracle.L.orc_close(d)


def _open_headers(oracle, pk):
    import ctypes as C
    hdr = pk[:3]
    blob = np.frombuffer(b"".join(hdr), dtype=np.uint8)
    offs = np.zeros(4, np.int64)
    offs[1:] = np.cumsum([len(p) for p in hdr])
    g3, f3, err = np.full(3, -1, np.int64), np.zeros(3, np.uint8), C.c_int(0)
    d = oracle.L.orc_open_packets(blob.ctypes.data, offs.ctypes.data, g3.ctypes.data, f3.ctypes.data, 3, C.byref(err))
    assert d
    return d


def _floor1_apply_case(oracle, gpu_ctx, pk, seed):
    """IFloor.Apply on random posts for every Floor1 of a setup, both block sizes; returns (ok items, refused items)."""
    import ctypes as C
    import nvorbis_amd as nv
    torch = _torch()
    rng = np.random.default_rng(seed)
    d = _open_headers(oracle, pk)
    st = nv.Stream(gpu_ctx, pk[0], pk[1], pk[2])
    n_ok = n_err = 0
    try:
        nfloors = oracle.L.orc_floor_info(d, 0, None, None, None)
        for fi in range(nfloors):
            t, pc, rg = st.floor_info(fi)
            ot, opc, org = C.c_int(), C.c_int(), C.c_int()
            oracle.L.orc_floor_info(d, fi, C.byref(ot), C.byref(opc), C.byref(org))
            assert (t, pc, rg) == (ot.value, opc.value, org.value)
            if t != 1:
                continue
            for n in sorted({st.block0, st.block1}):
                half, batch = n // 2, 96
                posts = np.zeros((batch, 64), np.int32)
                counts = np.full(batch, pc, np.int32)
                for b in range(batch):
                    kind = b % 4
                    if kind == 3 and b % 8 == 3:
                        counts[b] = 0  # floor without energy: Apply clears the vector
                        continue
                    hi = rg if kind < 2 else (rg * 3) // 2  # kind 2/3: values past the dB table's range now and then
                    posts[b, :2] = rng.integers(0, hi, 2)
                    v = rng.integers(0, rg if kind != 3 else 2 * rg, pc)
                    v[rng.random(pc) < (0.5 if kind != 1 else 0.1)] = 0  # unused posts
                    posts[b, 2:pc] = v[2:]
                res = rng.standard_normal((batch, half)).astype(np.float32)
                got = torch.from_numpy(res.copy()).cuda()
                status = st.floor1_apply(fi, n, posts, counts, got.data_ptr(), half)
                got = got.cpu().numpy()
                for b in range(batch):
                    ref = np.zeros(st.block1, np.float32)
                    ref[:half] = res[b]
                    p = np.ascontiguousarray(posts[b])
                    rc = oracle.L.orc_floor1_apply_posts(d, fi, n, p.ctypes.data, int(counts[b]), ref.ctypes.data, st.block1)
                    assert (rc == 0) == (status[b] == 0), (fi, n, b, rc, status[b])
                    if rc == 0:
                        n_ok += 1
                        assert np.array_equal(got[b].view(np.uint32), ref[:half].view(np.uint32)), (fi, n, b)
                    else:
                        n_err += 1
    finally:
        st.close()
        oracle.L.orc_close(d)
    return n_ok, n_err


@pytest.mark.parametrize("name", ["2test", "3test"])
def test_floor1_apply_operator_files(oracle, gpu_ctx, ogg_bytes, name):
    """Fine-grained ABI: IFloor.Apply (Floor1.cs:186-341) with the shipped files' floors on random posts == the oracle's
    floor1_apply, item by item; items whose curve leaves inverse_dB_table (quirk B-7) are refused by both."""
    import nvorbis_amd as nv
    pk, _, _ = nv.demux_ogg(ogg_bytes[name])
    n_ok, n_err = _floor1_apply_case(oracle, gpu_ctx, pk, 5)
    assert n_ok > 100


@pytest.mark.parametrize("name", ["mono_res0_small_blocks", "stereo_res1_coupled", "three_ch_res2_misaligned", "mono_8192"])
def test_floor1_apply_operator_synthetic(oracle, gpu_ctx, name):
    """The same for synthetic setups: random post X lists, multipliers 1..4, blocks 64..8192."""
    from tests import synth_stream as ss
    pk, _, _ = ss.filtered_stream(oracle, name, 4, 21)
    n_ok, n_err = _floor1_apply_case(oracle, gpu_ctx, pk, 9)
    assert n_ok > 50


def _residue_decode_case(oracle, gpu_ctx, pk, packet_ids, seed):
    """IResidue.Decode call by call: the cursor and residue index of every call Mapping.DecodePacket makes come from the
    oracle's trace of the full packet; each call is then replayed on both sides into the same random planes."""
    import ctypes as C
    import nvorbis_amd as nv
    torch = _torch()
    rng = np.random.default_rng(seed)
    d = _open_headers(oracle, pk)
    st = nv.Stream(gpu_ctx, pk[0], pk[1], pk[2])
    calls = 0
    kinds = set()
    try:
        ch, b1 = st.channels, st.block1
        scratch = np.zeros(ch * b1, np.float32)
        for i in packet_ids:
            a, b, c, e = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            if oracle.L.orc_decode_packet_block(d, pk[i], len(pk[i]), scratch.ctypes.data, C.byref(a), C.byref(b), C.byref(c), C.byref(e)) != 1:
                continue
            pos, idx, anyx = np.zeros(16, np.int32), np.zeros(16, np.int32), C.c_int()
            ncall = oracle.L.orc_last_residue_calls(d, pos.ctypes.data, idx.ctypes.data, 16, C.byref(anyx))
            for k in range(ncall):
                init = rng.standard_normal(ch * b1).astype(np.float32)
                ref = init.copy()
                rbits = C.c_int()
                rc = oracle.L.orc_residue_decode_at(d, int(idx[k]), pk[i], len(pk[i]), int(pos[k]), anyx.value, e.value, ref.ctypes.data,
                                                    C.byref(rbits))
                assert rc == 0
                got = torch.from_numpy(init.copy()).cuda()
                gbits = st.residue_decode(int(idx[k]), pk[i], int(pos[k]), e.value, got.data_ptr(), bool(anyx.value))
                got = got.cpu().numpy()
                half = e.value // 2
                g = got.reshape(ch, b1)[:, :half]
                r = ref.reshape(ch, b1)[:, :half]
                assert np.array_equal(g.view(np.uint32), r.view(np.uint32)), (i, k, float(np.abs(g - r).max()))
                # [n/2, block1) is scratch in the reference too (overwritten by the IMDCT or cleared): not compared
                if int(pos[k]) + rbits.value < len(pk[i]) * 8:
                    assert gbits == rbits.value, (i, k, gbits, rbits.value)
                calls += 1
                kinds.add((int(idx[k]), e.value, bool(np.any(g != init.reshape(ch, b1)[:, :half]))))
    finally:
        st.close()
        oracle.L.orc_close(d)
    return calls, kinds


@pytest.mark.parametrize("name", ["2test", "3test"])
def test_residue_decode_operator_files(oracle, gpu_ctx, ogg_bytes, name):
    """Fine-grained ABI: IResidue.Decode (Residue0.cs:119-201, Residue1.cs, Residue2.cs) on its own, bit-exact."""
    import nvorbis_amd as nv
    pk, _, _ = nv.demux_ogg(ogg_bytes[name])
    ids = list(range(3, min(len(pk), 30))) + list(range(30, len(pk), max(1, (len(pk) - 30) // 30)))
    calls, kinds = _residue_decode_case(oracle, gpu_ctx, pk, ids, 3)
    assert calls > 30 and any(k[2] for k in kinds)


@pytest.mark.parametrize("name", ["mono_res0_small_blocks", "stereo_res1_coupled", "three_ch_res2_misaligned", "six_ch_res2_4096",
                                  "two_submaps", "equal_blocks_overrun"])
def test_residue_decode_operator_synthetic(oracle, gpu_ctx, name):
    from tests import synth_stream as ss
    pk, _, _ = ss.filtered_stream(oracle, name, 24, 21)
    calls, kinds = _residue_decode_case(oracle, gpu_ctx, pk, range(3, len(pk)), 4)
    assert calls > 10 and any(k[2] for k in kinds)


@pytest.mark.parametrize("name", ["2test", "3test"])
def test_window_overlap_copy_operators(oracle, gpu_ctx, ogg_bytes, name):
    """Fine-grained ABI: Mode.Decode's window loop vs the oracle's CalcWindow table, OverlapBuffers and
    ClippingCopyBuffer / CopyBuffer vs their definitions (StreamDecoder.cs:391-415, 532-541; Utils.cs:30-43)."""
    import ctypes as C
    import nvorbis_amd as nv
    torch = _torch()
    rng = np.random.default_rng(8)
    pk, _, _ = nv.demux_ogg(ogg_bytes[name])
    d = _open_headers(oracle, pk)
    st = nv.Stream(gpu_ctx, pk[0], pk[1], pk[2])
    try:
        b0, b1, ch = st.block0, st.block1, st.channels
        nmodes = oracle.L.orc_mode_info(d, 0, None, None, None)
        assert st.mode_info(nmodes) is None
        for mi in range(nmodes):
            f, n, mp = C.c_int(), C.c_int(), C.c_int()
            oracle.L.orc_mode_info(d, mi, C.byref(f), C.byref(n), C.byref(mp))
            assert st.mode_info(mi) == (bool(f.value), n.value, mp.value)
            for prev in (0, 1):
                for nxt in (0, 1):
                    # Mode.cs:41-50: the flags pick the neighbours' block sizes for a long block; short blocks have one window
                    w = oracle.window(b1 if (prev or not f.value) else b0, n.value, b1 if (nxt or not f.value) else b0) if f.value \
                        else oracle.window(b0, n.value, b0)
                    x = rng.standard_normal((5, n.value + 8)).astype(np.float32)
                    g = torch.from_numpy(x.copy()).cuda()
                    st.window_apply(mi, prev, nxt, 5, g.data_ptr(), n.value + 8)
                    gpu_ctx.synchronize()  # asynchronous on the context's stream; torch reads on its own
                    want = x.copy()
                    want[:, :n.value] = x[:, :n.value] * w
                    assert np.array_equal(g.cpu().numpy().view(np.uint32), want.view(np.uint32)), (mi, prev, nxt)
        # OverlapBuffers
        prev = rng.standard_normal((ch, b1)).astype(np.float32)
        nxt = rng.standard_normal((ch, b1)).astype(np.float32)
        for (ps, pe, ns) in [(b1 // 2, b1 * 3 // 4, 0), (b1 * 3 // 4 - b0 // 4, b1 * 3 // 4 + b0 // 4, b1 // 4 - b0 // 4), (7, 7, 3), (0, b1, 0)]:
            gp, gn = torch.from_numpy(prev).cuda(), torch.from_numpy(nxt.copy()).cuda()
            gpu_ctx.overlap_buffers(gp.data_ptr(), gn.data_ptr(), ps, pe, ns, ch, b1)
            gpu_ctx.synchronize()
            want = nxt.copy()
            want[:, ns:ns + pe - ps] = nxt[:, ns:ns + pe - ps] + prev[:, ps:pe]
            assert np.array_equal(gn.cpu().numpy().view(np.uint32), want.view(np.uint32))
        # ClippingCopyBuffer / CopyBuffer
        planes = (rng.standard_normal((ch, b1)) * 0.6).astype(np.float32)
        planes[0, 5], planes[ch - 1, 9] = np.float32(0.99999994), np.float32(-0.99999994)  # the bounds themselves are not clipped
        gp = torch.from_numpy(planes).cuda()
        for clip in (True, False):
            for (s0, cnt) in [(0, b1), (3, 1000 if b1 > 1100 else 40), (11, 0)]:
                out = _dev_zeros(max(cnt, 1) * ch)
                clipped = gpu_ctx.copy_buffer(gp.data_ptr(), s0, cnt, ch, b1, out.data_ptr(), clip)
                seg = planes[:, s0:s0 + cnt]
                lim = np.float32(0.99999994)
                want = np.clip(seg, -lim, lim) if clip else seg
                assert np.array_equal(out.cpu().numpy()[:cnt * ch].view(np.uint32), np.ascontiguousarray(want.T).reshape(-1).view(np.uint32))
                assert clipped == bool(clip and cnt and (np.abs(seg) > lim).any())
        quiet = torch.from_numpy((planes * 0.1).astype(np.float32)).cuda()
        out = _dev_zeros(b1 * ch)
        assert gpu_ctx.copy_buffer(quiet.data_ptr(), 0, b1, ch, b1, out.data_ptr(), True) is False
    finally:
        st.close()
        oracle.L.orc_close(d)


def test_floor0_apply_operator(oracle, gpu_ctx):
    """Fine-grained ABI: IFloor.Apply for Floor0 (Floor0.cs:152-212) on random LSP coefficients; double-precision
    cos/sqrt/exp rounded to float on both sides (device ocml, host glibc): identical bit for bit on this device (see
    test_floor0_within_tolerance); empty floors cleared."""
    import ctypes as C
    import nvorbis_amd as nv
    from tests import synth_stream as ss
    torch = _torch()
    rng = np.random.default_rng(12)
    pk, _, _ = ss.filtered_stream(oracle, "floor0_stereo", 4, 21)
    d = _open_headers(oracle, pk)
    st = nv.Stream(gpu_ctx, pk[0], pk[1], pk[2])
    try:
        nfloors = oracle.L.orc_floor_info(d, 0, None, None, None)
        done = 0
        for fi in range(nfloors):
            t, order, _ = st.floor_info(fi)
            ot, oo = C.c_int(), C.c_int()
            oracle.L.orc_floor_info(d, fi, C.byref(ot), C.byref(oo), None)
            assert (t, order) == (ot.value, oo.value)
            if t != 0:
                continue
            for n in sorted({st.block0, st.block1}):
                half, batch = n // 2, 40
                amps = rng.uniform(0.25, 6.0, batch).astype(np.float32)
                amps[::7] = 0.0
                coeffs = np.sort(rng.uniform(0.05, 3.1, (batch, order + 3)), axis=1).astype(np.float32)
                res = rng.standard_normal((batch, half)).astype(np.float32)
                got = torch.from_numpy(res.copy()).cuda()
                status = st.floor0_apply(fi, n, amps, coeffs, got.data_ptr(), half)
                got = got.cpu().numpy()
                assert not status.any()
                exact = total = 0
                for b in range(batch):
                    ref = np.zeros(st.block1, np.float32)
                    ref[:half] = res[b]
                    cf = np.ascontiguousarray(coeffs[b])
                    assert oracle.L.orc_floor0_apply_coeffs(d, fi, n, float(amps[b]), cf.ctypes.data, ref.ctypes.data, st.block1) == 0
                    r = ref[:half]
                    if amps[b] <= 0:
                        assert not got[b].any() and not r.any()
                        continue
                    fin = np.isfinite(r)
                    assert np.array_equal(got[b][~fin].view(np.uint32), r[~fin].view(np.uint32))  # overflowed curves: same inf
                    g64, r64 = got[b][fin].astype(np.float64), r[fin].astype(np.float64)
                    assert np.all(np.abs(g64 - r64) <= 2e-5 * np.abs(r64) + 1e-30), (fi, n, b)
                    exact += int((got[b].view(np.uint32) == r.view(np.uint32)).sum())
                    total += half
                    done += 1
                assert exact == total, (exact, total)
        assert done > 40
    finally:
        st.close()
        oracle.L.orc_close(d)


def _chunked_gpu(gpu_ctx, pk, gr, fl, world, gpu_parse, clip=True, batch_frames=64):
    from nvorbis_amd.corpus import decode_stream_chunk, plan_stream_chunks
    chunks = plan_stream_chunks(pk, gr, fl, world, gpu_ctx if gpu_parse else None)
    parts, clipped = [], False
    for i, c in enumerate(chunks):
        pcm, cl = decode_stream_chunk(gpu_ctx, pk, gr, fl, c, i == len(chunks) - 1, batch_frames=batch_frames, gpu_parse=gpu_parse,
                                      clip=clip)
        parts.append(pcm)
        clipped |= cl
    return (np.concatenate(parts) if parts else np.zeros(0, np.float32)), chunks, clipped


@pytest.mark.parametrize("name", ["1test", "2test", "3test", "issue6test"])
@pytest.mark.parametrize("gpu_parse", [False, True])
def test_stream_chunks_on_gpu_equal_serial(oracle, gpu_ctx, ogg_bytes, name, gpu_parse):
    """SURVEY 8e, one stream over several GPUs: every chunk of the plan decoded by its own nvh_stream (lead-in packet,
    then the serial decoder's position state) -- here one after the other on one GPU -- concatenates to the serial
    decode and to the oracle, bit for bit, including issue6test's non-zero start position and end-of-stream drain."""
    import nvorbis_amd as nv
    pk, gr, fl = nv.demux_ogg(ogg_bytes[name])
    ref, info = oracle.decode_ogg(ogg_bytes[name])
    for world in (2, 5):
        got, chunks, clipped = _chunked_gpu(gpu_ctx, pk, gr, fl, world, gpu_parse)
        assert len(chunks) == world
        assert got.size == ref.size
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (name, world)
        assert clipped == info["has_clipped"]


@pytest.mark.parametrize("name", ["stereo_res1_coupled", "three_ch_res2_misaligned", "equal_blocks_overrun", "longcode_res2"])
@pytest.mark.parametrize("consistent", [True, False])
def test_stream_chunks_synthetic(oracle, gpu_ctx, name, consistent):
    """The same on random-bit streams, including inconsistent window flags: cuts are only placed where the lead-in
    packet alone reproduces the tail the next packet overlaps with, so the result is still the serial one."""
    from tests import synth_stream as ss
    pk, gr, fl = ss.filtered_stream(oracle, name, 150, 31 + int(consistent), consistent_windows=consistent)
    ref, _ = oracle.decode_packets(pk, gr, fl)
    for world in (2, 4):
        got, chunks, _ = _chunked_gpu(gpu_ctx, pk, gr, fl, world, False)
        assert len(chunks) >= 2
        assert got.size == ref.size
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (name, consistent, world)


def _seek_outcome(nv, rd, t, buf):
    """(class, samples, position after) of SeekTo(t) + one ReadSamples on the product, classes named after the oracle's codes."""
    try:
        rd.SeekTo(t)
    except IndexError:
        return -2, None, rd.SamplePosition            # ArgumentOutOfRangeException
    except nv.native.NvhError as e:
        return e.code, None, None                    # InvalidDataException (-1) / the reference spins or faults (-3)
    except RuntimeError:
        return -6, None, None                        # InvalidOperationException
    at = rd.SamplePosition
    n = rd.ReadSamples(buf, 0, buf.size)
    return 0, (at, buf[:n].copy()), rd.SamplePosition


@pytest.mark.parametrize("name", ["1test", "2test", "3test", "issue6test"])
@pytest.mark.parametrize("gpu_parse", [False, True])
def test_seek_matches_the_reference_decoder(oracle, ogg_bytes, name, gpu_parse):
    """StreamDecoder.SeekTo (StreamDecoder.cs:562-628) over the reference's page-level search (tests/test_seek_pages.py): the same
    sequence of seeks and reads on the product (VorbisReader over the C ABI) and on the oracle's restatement (orc_seek_to) gives
    the same samples, positions and exception classes -- for targets at packet and page boundaries, inside long and short blocks,
    on the first data page (where the reference lands early or, for a roll-forward longer than the packet, never returns from
    Read: RUNTIME on both sides), on the last page (InvalidDataException where its granule position is trimmed), past the end.
    Away from those pages the samples are also the serial decode's."""
    import nvorbis_amd as nv
    data = ogg_bytes[name]
    ref, info = oracle.decode_ogg(data)
    ch = info["channels"]
    d = oracle.open_ogg(data)
    rd = nv.VorbisReader(data, device=0, batch_frames=64, gpu_parse=gpu_parse)
    try:
        full = rd.read_all()
        assert np.array_equal(full.view(np.uint32), ref.view(np.uint32))
        got_all = oracle._drain(oracle.open_ogg(data), True, 4096, False)[0]
        assert got_all.size == ref.size
        end = rd.SamplePosition
        first = end - ref.size // ch
        total = rd.TotalSamples
        assert total == oracle.L.orc_total_samples(d)
        # bring the oracle decoder to the same state (everything read)
        tmp = np.zeros(1 << 16, np.float32)
        while oracle.L.orc_read_samples(d, tmp.ctypes.data, tmp.size, 0, tmp.size - tmp.size % ch) > 0:
            pass
        assert oracle.L.orc_sample_position(d) == end
        rng = np.random.default_rng(17)
        targets = [0, 1, 64, 127, 128, 129, 1000, 1024, 2048, 5000, total - 1, total - 700, total, total + 1, (first + end) // 2]
        targets += [int(t) for t in rng.integers(0, total, 40)]
        buf = np.empty(5000 * ch, np.float32)
        seen = {}
        serial_ok = 0
        for t in targets:
            rc, smp, pos_after = oracle.seek_and_read(d, t, buf.size)
            cls, mine, my_pos = _seek_outcome(nv, rd, t, buf)
            if rc == 0 and isinstance(smp, int):       # the seek went through, the managed Read would spin
                assert smp == -3 and cls == -3, (t, smp, cls)
                seen["spin"] = seen.get("spin", 0) + 1
                continue
            assert cls == rc, (name, t, cls, rc)
            seen[rc] = seen.get(rc, 0) + 1
            if rc != 0:
                continue
            at, pcm = mine
            assert at == t and pcm.size == smp.size, (t, at, pcm.size, smp.size)
            assert np.array_equal(pcm.view(np.uint32), smp.view(np.uint32)), t
            assert my_pos == pos_after == t + pcm.size // ch
            want = ref[(t - first) * ch:(t - first) * ch + pcm.size] if t >= first else None
            if want is not None and want.size == pcm.size and np.array_equal(pcm.view(np.uint32), want.view(np.uint32)):
                serial_ok += 1
        assert seen.get(0, 0) >= 20 and serial_ok >= 10, (seen, serial_ok)
        assert seen.get(-2, 0) >= 1                      # past the end
        # read on to the end of the stream after a seek: same samples, then end of stream on both sides
        t = int((first + end) // 2)
        assert oracle.L.orc_seek_to(d, t) == 0
        rd.SeekTo(t)
        tail = rd.read_all()
        chunks = []
        while True:
            n = oracle.L.orc_read_samples(d, tmp.ctypes.data, tmp.size, 0, tmp.size - tmp.size % ch)
            if n <= 0:
                break
            chunks.append(tmp[:n].copy())
        otail = np.concatenate(chunks)
        assert np.array_equal(tail.view(np.uint32), otail.view(np.uint32))
        assert rd.IsEndOfStream and rd.ReadSamples(buf, 0, buf.size) == 0
        # setters and origins
        mid = (first + end) // 2
        rd.SamplePosition = mid
        assert rd.SamplePosition == mid
        rd.SeekTo(total // 3, "end")
        assert rd.SamplePosition == total - total // 3
        rd.SeekTo(50, "current")  # the reference computes SamplePosition - value (StreamDecoder.cs:573)
        assert rd.SamplePosition == total - total // 3 - 50
        secs = 0.25 * rd.TotalTime
        rd.TimePosition = secs
        assert rd.SamplePosition == int(rd.SampleRate * secs)
        # back to the very beginning: position 0 restarts the stream
        rd.SeekTo(0)
        again = rd.read_all()
        assert oracle.L.orc_seek_to(d, 0) == 0
        o_again = oracle._drain(d, True, 4096, False)[0]
        d = None
        assert np.array_equal(again.view(np.uint32), o_again.view(np.uint32))
        for bad in (-1, end + 10_000_000):
            with pytest.raises(IndexError):
                rd.SeekTo(bad)
    finally:
        rd.close()
        if d is not None:
            oracle.L.orc_close(d)


def test_reader_switches_between_logical_streams(oracle, ogg_bytes):
    """VorbisReader over a chained + multiplexed container: StreamCount, SwitchStreams (VorbisReader.cs:290-305) with the
    clipping setting carried over and the changed-format return value; each logical stream decodes to the PCM of the file
    it came from, and a stream that was left half read resumes where it was."""
    import nvorbis_amd as nv
    from tests.test_host_logic import _ogg_pages
    pa, pb = _ogg_pages(ogg_bytes["2test"]), _ogg_pages(ogg_bytes["3test"])
    mux = b"".join((pa[i] if i < len(pa) else b"") + (pb[i] if i < len(pb) else b"") for i in range(max(len(pa), len(pb))))
    data = mux + ogg_bytes["issue6test"]  # streams: 2test (mono), 3test (stereo), issue6test (stereo)
    want = [oracle.decode_ogg(ogg_bytes[n])[0] for n in ("2test", "3test", "issue6test")]
    rd = nv.VorbisReader(data, device=0)
    try:
        assert rd.StreamCount == 3 and rd.StreamIndex == 0 and rd.Channels == 1
        head = np.empty(5000, np.float32)
        n0 = rd.ReadSamples(head, 0, head.size)
        assert np.array_equal(head[:n0].view(np.uint32), want[0][:n0].view(np.uint32))
        rd.ClipSamples = False
        assert rd.SwitchStreams(1) is True and rd.Channels == 2 and rd.ClipSamples is False
        ref_noclip = oracle.decode_ogg(ogg_bytes["3test"], clip=False)[0]
        got = rd.read_all()
        assert np.array_equal(got.view(np.uint32), ref_noclip.view(np.uint32))
        assert rd.SwitchStreams(2) is False  # stereo 44.1 kHz again
        rd.ClipSamples = True
        assert np.array_equal(rd.read_all().view(np.uint32), want[2].view(np.uint32))
        assert rd.SwitchStreams(2) is False and rd.SwitchStreams(0) is True
        rest = rd.read_all()  # the first stream resumes after the 5000 samples read before
        assert np.array_equal(rest.view(np.uint32), want[0][n0:].view(np.uint32))
        with pytest.raises(IndexError):
            rd.SwitchStreams(3)
    finally:
        rd.close()


@pytest.mark.parametrize("gpu_parse", [False, True])
def test_pipelined_read_back_is_the_same_pcm(oracle, gpu_ctx, ogg_bytes, gpu_parse):
    """nvh_stream_synth_begin / _end (two batches outstanding, the PCM of one travelling to the host while the next is pushed,
    parsed and synthesised): the concatenated PCM is the oracle's, bit for bit, for a file with both block sizes and the
    end-of-stream trim, with small and large batches; misuse (a third begin, an end without a begin, the synchronous call in
    between) is refused with NVH_ERR_ARGUMENT and leaves the outstanding batches intact."""
    import nvorbis_amd as nv
    pk, gr, fl = nv.demux_ogg(ogg_bytes["3test"])
    ref, _ = oracle.decode_packets(pk, gr.tolist(), fl.tolist())
    for per_batch in (37, 500):
        st = nv.Stream(gpu_ctx, pk[0], pk[1], pk[2])
        try:
            st.set_gpu_parse(gpu_parse)
            chunks, outstanding, i = [], 0, 3
            while i < len(pk) or outstanding:
                if i < len(pk) and outstanding < 2:
                    j = min(i + per_batch, len(pk))
                    for k in range(i, j):
                        st.push_packet(pk[k], int(gr[k]), int(fl[k]))
                    if j == len(pk):
                        st.push_end()
                    i = j
                    st.synth_begin()
                    outstanding += 1
                    if outstanding == 2 and not chunks:  # misuse while two batches are in flight
                        with pytest.raises(nv.native.NvhError):
                            st.synth_begin()
                        with pytest.raises(nv.native.NvhError):
                            st.synth_host()
                    continue
                chunks.append(st.synth_end().copy())
                outstanding -= 1
            with pytest.raises(nv.native.NvhError):
                st.synth_end()
            got = np.concatenate(chunks)
            assert got.size == ref.size and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (gpu_parse, per_batch)
        finally:
            st.close()


def test_pipelined_read_back_survives_reset_and_misuse(oracle, gpu_ctx, ogg_bytes):
    """The Python side of the begin / end pairing follows the native flight slots: a reset with ONE batch outstanding
    (nvh_stream_reset abandons it and rewinds both native slot indices) must not leave the next begin and end on different
    page-locked buffers, a refused begin (two outstanding, larger third batch) must not free the buffer the oldest batch
    is still being copied into, and an end with nothing outstanding must not flip the pairing."""
    import nvorbis_amd as nv
    pk, gr, fl = nv.demux_ogg(ogg_bytes["2test"])
    ref, _ = oracle.decode_packets(pk, gr.tolist(), fl.tolist())
    st = nv.Stream(gpu_ctx, pk[0], pk[1], pk[2])
    try:
        with pytest.raises(nv.native.NvhError):
            st.synth_end()  # nothing outstanding
        # one batch outstanding, then ResetDecoder
        for k in range(3, 40):
            st.push_packet(pk[k], int(gr[k]), int(fl[k]))
        st.synth_begin()
        st.reset()
        st.set_position_state(False, 0)  # ResetDecoder leaves _currentPosition alone (StreamDecoder.cs:294-304): start over as a new decoder would
        # the whole stream again in three batches, two of them in flight, the third (larger) refused while they are
        cuts = [3, 30, 60, len(pk)]
        for a, b in zip(cuts[:2], cuts[1:3]):
            for k in range(a, b):
                st.push_packet(pk[k], int(gr[k]), int(fl[k]))
            st.synth_begin()
        for k in range(cuts[2], cuts[3]):
            st.push_packet(pk[k], int(gr[k]), int(fl[k]))
        st.push_end()
        with pytest.raises(nv.native.NvhError):
            st.synth_begin()
        chunks = [st.synth_end().copy(), st.synth_end().copy()]
        st.synth_begin()
        chunks.append(st.synth_end().copy())
        with pytest.raises(nv.native.NvhError):
            st.synth_end()
        got = np.concatenate(chunks)
        assert got.size == ref.size
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    finally:
        st.close()
