"""Shared test helpers: workload generators and the oracle-side driver that
plays the role vpz_decoder_synth plays on the GPU."""
import ctypes as C

import numpy as np

PKT_BLOCK_FLAG, PKT_PREV_FLAG, PKT_NEXT_FLAG, PKT_EOS = 0x01, 0x02, 0x04, 0x08
PKT_NOT_DECODED, PKT_INTERLEAVED, PKT_NO_FLOOR = 0x10, 0x20, 0x40

# X list of a libvorbis 44.1 kHz long-block floor1 (29 posts, the shape 3test.ogg's long floor has)
LONG_XLIST = [0, 1024, 93, 23, 372, 6, 46, 186, 750, 14, 33, 65, 130, 260, 556, 3, 10, 18, 28, 39, 55,
              79, 111, 158, 220, 312, 464, 650, 850]
SHORT_XLIST = [0, 128, 12, 46, 4, 8, 16, 23, 33, 70, 2, 6, 10, 14, 19, 28, 39, 58, 90]


def markov_block_flags(frames, seed, p_ls=0.1, p_sl=0.3, start_long=True):
    """Config 3 block-flag chain: p(long->short)=0.1, p(short->long)=0.3; returns the packet flag
    bytes with prev/next window flags made mutually consistent (StreamDecoder.cs:654,778)."""
    rng = np.random.default_rng(seed)
    u = rng.random(frames)
    bf = np.zeros(frames, dtype=np.uint8)
    cur = 1 if start_long else 0
    for i in range(frames):
        bf[i] = cur
        cur = (0 if u[i] < p_ls else 1) if cur else (1 if u[i] < p_sl else 0)
    prev = np.concatenate([[1], bf[:-1]])
    nxt = np.concatenate([bf[1:], [1]])
    return (bf * PKT_BLOCK_FLAG | prev * PKT_PREV_FLAG * bf | nxt * PKT_NEXT_FLAG * bf).astype(np.uint8)


def gaussian_spectra(shape, seed, sigma=2.0 ** -8):
    return (np.random.default_rng(seed).standard_normal(shape) * sigma).astype(np.float32)


PKT_RESYNC = 0x80


class OracleStream:
    """One reference StreamDecoder, restated: the oracle's stream state plus what Read()'s `while (idx == 0)` loop does
    around ReadNextPacket (StreamDecoder.cs:418-498).  Packets are dicts with keys flags, granule (default -1), mapping
    (default 0), residue (np [channels*half] as laid out for the ABI), posts (np [channels, <=64]), post_count
    (np [channels]), for type-0 floors f0_amp / f0_coeff."""

    def __init__(self, orc, channels, size0, size1, floors=(), mappings=(), clip=False, interleave=False, state=None):
        self.orc, self.L = orc, orc.lib()
        self.channels, self.size0, self.size1 = channels, size0, size1
        self.floors, self.mappings, self.clip, self.interleave = floors, mappings, clip, interleave
        self.st = state if state is not None else self.L.orc_stream_create(channels, size0, size1)
        self.ofl = [orc.floor1_init(*f) if not isinstance(f, dict) else None for f in floors]
        self.eos_seen = False
        self.mismatches = 0

    def close(self):
        if self.st is not None:
            self.L.orc_stream_destroy(self.st)
            self.st = None

    def take(self):
        """Hands out everything readable, like repeated Read calls; returns [channels, n] or None."""
        L, st, channels = self.L, self.st, self.channels
        n = L.orc_stream_available(st)
        if n <= 0:
            return None
        if self.interleave:
            buf = np.zeros((n, channels), dtype=np.float32)
            L.orc_stream_store(st, buf.ctypes.data_as(C.POINTER(C.c_float)), 0, n, 0, 1, int(self.clip))
            return buf.T.copy()
        buf = np.zeros((channels, n), dtype=np.float32)
        L.orc_stream_store(st, buf.ctypes.data_as(C.POINTER(C.c_float)), 0, n, n, 0, int(self.clip))
        return buf

    def read_next_packet(self, pk):
        """DecodeNextPacket + ReadNextPacket for one packet (StreamDecoder.cs:640-762); returns ReadNextPacket's result
        (1 accepted, 0 no packet, -1 where OverlapBuffers throws)."""
        orc, L, st = self.orc, self.L, self.st
        channels, size0, size1, floors, mappings = self.channels, self.size0, self.size1, self.floors, self.mappings
        flags = pk["flags"]
        eos = 1 if flags & PKT_EOS else 0
        if flags & PKT_RESYNC:
            L.orc_stream_mark_resync(st)  # :718-722, before the packet's first bit is looked at
        if flags & PKT_NOT_DECODED:
            L.orc_stream_read_next_packet(st, 0, None, -1, eos)
            return 0
        bf = 1 if flags & PKT_BLOCK_FLAG else 0
        n = size1 if bf else size0
        half = n // 2
        info = orc.packet_info(size0, size1, bf, bool(flags & PKT_PREV_FLAG), bool(flags & PKT_NEXT_FLAG))
        res = np.asarray(pk["residue"], dtype=np.float32)
        if flags & PKT_INTERLEAVED:
            res = res.reshape(half, channels).T.copy()
        else:
            res = res.reshape(channels, half)
        if flags & PKT_NO_FLOOR:
            pcm = np.stack([orc.mdct_reverse(res[c][None, :], n)[0] for c in range(channels)])
        elif any(isinstance(f, dict) for f in floors):
            # mixed floor types: Mapping.cs:166-195 step by step (type-0 floors: Floor0.cs:164-225)
            m = mappings[pk.get("mapping", 0)]
            res = res.copy()
            for mag, ang in reversed(m.get("coupling", [])):
                res[mag], res[ang] = orc.apply_coupling(res[mag], res[ang])
            pcm = np.zeros((channels, n), dtype=np.float32)
            for c in range(channels):
                fl = floors[m.get("channel_floor", [0] * channels)[c]]
                if isinstance(fl, dict):
                    amp = float(pk["f0_amp"][c])
                    if amp == 0:
                        continue  # ExecuteChannel false (Floor0.cs:22)
                    spec = orc.floor0_apply(fl["order"], fl["rate"], fl["bark_map_size"], fl["amp_bits"], fl["amp_ofs"],
                                            pk["f0_coeff"][c][:fl["order"]], amp, n, res[c])
                else:
                    if pk["post_count"][c] == 0:
                        continue
                    spec = orc.floor1_apply(orc.floor1_init(*fl), pk["posts"][c], int(pk["post_count"][c]), n, res[c])
                pcm[c] = orc.mdct_reverse(spec[None, :], n)[0]
        else:
            m = mappings[pk.get("mapping", 0)]
            pcm = orc.mapping_synth(channels, n, res, self.ofl, m.get("channel_floor", [0] * channels),
                                    pk["posts"], pk["post_count"], m.get("coupling", []))
        p = L.orc_stream_next_buffer(st)
        view = np.ctypeslib.as_array(p, shape=(channels, size1))
        view[:] = 0
        view[:, :n] = pcm
        return L.orc_stream_read_next_packet(st, 1, C.byref(info), int(pk.get("granule", -1)), eos)

    def feed(self, pk):
        """One iteration of Read()'s loop for a packet: returns the samples it made readable ([channels, n] or None)."""
        if self.eos_seen and self.L.orc_stream_available(self.st) == 0:
            return None  # Read(): nothing more is read after EOS (StreamDecoder.cs:441-447)
        rc = self.read_next_packet(pk)
        eos = bool(pk["flags"] & PKT_EOS)
        if pk["flags"] & PKT_NOT_DECODED:
            if eos:
                self.eos_seen = True
                self.L.orc_stream_drain_eos(self.st)
                return self.take()
            return None
        if eos:
            self.eos_seen = True
        if rc < 0:
            # OverlapBuffers would throw (StreamDecoder.cs:777-778): that Read fails, the packet is
            # consumed, the decoder state stays as it was
            self.mismatches += 1
            return None
        return self.take()

    @property
    def position(self):
        return self.L.orc_stream_position(self.st)

    @property
    def has_clipped(self):
        return bool(self.L.orc_stream_has_clipped(self.st))


def oracle_decode(orc, channels, size0, size1, packets, floors=(), mappings=(), clip=False,
                  interleave=False, state=None, keep_state=False):
    """Runs one stream through the oracle (see OracleStream for the packet dicts).  Returns PCM [channels, T] or
    [T, channels], the position and the clip flag."""
    # `state`: continue on an oracle stream a previous call kept (keep_state=True returns it as a 4th value,
    # e.g. to put an orc_stream_reset between two calls)
    s = OracleStream(orc, channels, size0, size1, floors, mappings, clip, interleave, state=state)
    chunks = []
    for pk in packets:
        got = s.feed(pk)
        if got is not None:
            chunks.append(got)
    pos, clipped, st = s.position, s.has_clipped, s.st
    if not keep_state:
        s.close()
    pcm = np.concatenate(chunks, axis=1) if chunks else np.zeros((channels, 0), dtype=np.float32)
    oracle_decode.last_mismatches = s.mismatches
    if keep_state:
        return (pcm.T.copy() if interleave else pcm), pos, clipped, st
    return (pcm.T.copy() if interleave else pcm), pos, clipped


def random_posts(rng, xlist, multiplier, n_ch, silent_prob=0.0):
    """Raw floor1 posts as `Floor1.Unpack` leaves them: two absolute values then residuals."""
    rng_range = {1: 256, 2: 128, 3: 86, 4: 64}[multiplier]
    posts = np.zeros((n_ch, 64), dtype=np.int16)
    counts = np.zeros(n_ch, dtype=np.uint8)
    for c in range(n_ch):
        if rng.random() < silent_prob:
            continue
        counts[c] = len(xlist)
        posts[c, 0] = rng.integers(rng_range // 4, rng_range // 2)
        posts[c, 1] = rng.integers(rng_range // 8, rng_range // 3)
        vals = rng.integers(0, 12, size=len(xlist) - 2)
        vals[rng.random(len(vals)) < 0.35] = 0
        posts[c, 2:len(xlist)] = vals
    return posts, counts


def packets_for_oracle(ogg, pk, residue, posts, counts):
    """Converts the front end's batch arrays (vorbispizza_amd.front.OggVorbisFile.decode_packets) into
    the per-packet dicts oracle_decode takes."""
    C_ = ogg.channels
    out = []
    for i in range(len(pk)):
        flags = int(pk["flags"][i])
        d = {"flags": flags, "granule": int(pk["granule"][i]), "mapping": int(pk["mapping"][i])}
        if not flags & PKT_NOT_DECODED:
            half = (ogg.block_size1 if flags & PKT_BLOCK_FLAG else ogg.block_size0) // 2
            off = int(pk["residue_offset"][i])
            d["residue"] = residue[off: off + C_ * half]
            d["posts"] = posts[i * C_:(i + 1) * C_]
            d["post_count"] = counts[i * C_:(i + 1) * C_]
            if getattr(ogg, "floor0_data", None) is not None:
                d["f0_amp"] = ogg.floor0_data[0][i * C_:(i + 1) * C_]
                d["f0_coeff"] = ogg.floor0_data[1][i * C_:(i + 1) * C_]
        out.append(d)
    return out


def floor0_safe_amp(coeff, bark_map_size, amp_ofs):
    """Largest amp for which Floor0's curve stays <= 0 dB: amp_ofs * min_k sqrt(p(k) + q(k))."""
    c = 2.0 * np.cos(coeff.astype(np.float64))
    w = 2.0 * np.cos(np.pi / bark_map_size * np.arange(bark_map_size))
    p = np.full_like(w, 0.5)
    q = np.full_like(w, 0.5)
    order = len(c)
    j = 1
    while j < order:
        q *= w - c[j - 1]
        p *= w - c[j]
        j += 2
    if j == order:
        q *= w - c[j - 1]
        p *= p * (4.0 - w * w)
        q *= q
    else:
        p *= p * (2.0 - w)
        q *= q * (2.0 + w)
    return float(amp_ofs * np.sqrt(np.maximum(p + q, 1e-30)).min())


# ---- all-long stereo streams through the chained by-length route (test_full_size_gpu.py, test_chained_route_gpu.py)

ALL_LONG = PKT_BLOCK_FLAG | PKT_PREV_FLAG | PKT_NEXT_FLAG

_CUT_LINE = (r"\[vpz host\] cut: [^,]+, by (?P<by>cost|length), R (?P<R>\d+), target (?P<target>-?\d+) eighths, (?P<runs>\d+) runs "
             r"for -?\d+ slots, .*?heavy below (?P<heavy>-?\d+), .*?chained (?P<chained>\d+), runs filled by (?P<fill>the pool|the calling thread) on (?P<fill_threads>\d+) threads, "
             r"chain sweep on (?P<chain_threads>\d+) threads")
_CALL_LINE = r"\[vpz host\] packets (?P<packets>\d+): route (?P<route>\w+), .*? pass1 [\d.]+ us \((?P<pass1>parallel|serial)\)"


def host_profile(err):
    """The route of ONE synth call as VPZ_HOST_PROFILE=1 prints it on stderr: a dict of the cut line's and the call line's fields
    (R, runs, chained, fill_threads, chain_threads as ints), or an AssertionError naming what was printed."""
    import re
    cut, call = re.findall(_CUT_LINE, err), re.findall(_CALL_LINE, err)
    assert len(cut) == 1 and len(call) == 1, "expected one cut line and one call line, got:\n" + err[-2000:]
    m = re.search(_CUT_LINE, err).groupdict()
    m.update(re.search(_CALL_LINE, err).groupdict())
    for k in ("R", "runs", "chained", "fill_threads", "chain_threads", "packets", "target", "heavy"):
        m[k] = int(m[k])
    return m


def resolved_host_threads():
    """What a decoder left at host_threads = 0 resolves to: VPZ_HOST_THREADS if set, else the CPUs this process may run on
    divided by LOCAL_WORLD_SIZE, 1 ... 16 (vpz_decoder_set_host_threads)."""
    import os
    if int(os.environ.get("VPZ_HOST_THREADS", "0") or 0) > 0:
        return int(os.environ["VPZ_HOST_THREADS"])
    n = len(os.sched_getaffinity(0)) // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1") or 1))
    return max(1, min(n, 16))


def by_length_runs(frames_per_stream, R):
    """The runs of a cut by length without skew: per stream in this call, runs of R frames and a partial one.  Returns
    [(stream, index within the stream's runs, frames in the run)] in launch order."""
    runs = []
    for s, n in enumerate(frames_per_stream):
        for j, f0 in enumerate(range(0, n, R)):
            runs.append((s, j, min(R, n - f0)))
    return runs


def cost_codes(packets, dual):
    """DESIGN 4.3 / 4.7, the cost of a stream's packets IN ONE CALL ([(flags, mapping)] in order), in eighths of a long block's pass:
    a long block 8; a short block alone or at the head of a batch 8 on the stereo / pair routes (`dual`) and 6 in group mode; a short
    block that rides in a batch 2 / 3.  A short block may ride (`ok`) when it has a predecessor in the call, on the stereo routes
    always, in group mode when it is Residue2-interleaved and not already floored; it joins its predecessor's batch when that may
    ride too, is short and has the same mapping (and both are floored or both are not: counted in the total only); a batch holds
    eight blocks.  Returns ([(is_short, ok, same mapping as a short predecessor)], the stream's total cost)."""
    w_short, w_member = (8, 2) if dual else (6, 3)
    codes, units, pos, prev_ok = [], 0, -1, False
    for i, (fl, mp) in enumerate(packets):
        short = not fl & PKT_BLOCK_FLAG
        ok = same = link = False
        if i > 0:
            pfl, pmp = packets[i - 1]
            p_short = not pfl & PKT_BLOCK_FLAG
            ok = short and not (fl | pfl) & PKT_NOT_DECODED and (dual or bool(fl & PKT_INTERLEAVED and not fl & PKT_NO_FLOOR))
            same = ok and mp == pmp and p_short
            link = same and prev_ok and not (fl ^ pfl) & PKT_NO_FLOOR
        pos = (pos + 1 if link else 0) if ok else -1
        units += w_member if ok and pos & 7 else (w_short if short else 8)
        codes.append((short, ok, same))
        prev_ok = ok
    return codes, units


def by_cost_runs(packets_per_stream, target, r_max, dual, heavy=-1):
    """The runs of a cut by cost: a run takes frames while its cost stays within the target and it holds fewer
    than r_max frames (the descriptor area), at least one; inside a run the batches start over.  `heavy` >= 0 (the stereo routes'
    skew): a run that starts below that much of the call's cost gets target + 2.5 %, the others target - 2.5 %.  Returns
    [(stream, index within the stream's runs, frames, cost, whether the frame cap and not the cost ended the run)]."""
    w_short, w_member = (8, 2) if dual else (6, 3)
    runs, prefix = [], 0
    for s, packets in enumerate(packets_per_stream):
        codes, total = cost_codes(packets, dual)
        f0, j, before = 0, 0, 0
        while f0 < len(codes):
            t = target
            if heavy >= 0:
                t += target * 25 // 1000 if prefix + before < heavy else -(target * 25 // 1000)
            n, units, pos, prev_ok, capped = 0, 0, -1, False, False
            while f0 + n < len(codes):
                short, ok, same = codes[f0 + n]
                link = ok and prev_ok and same
                p = (pos + 1 if link else 0) if ok else -1
                u = w_member if ok and p & 7 else (w_short if short else 8)
                if n > 0 and units + u > t:
                    break
                if n == r_max:
                    capped = True
                    break
                units, pos, prev_ok, n = units + u, p, ok, n + 1
            runs.append((s, j, n, units, capped))
            f0, j, before = f0 + n, j + 1, before + units
        prefix += total
    return runs


def expected_chained(frames_per_stream, R, trimmed=(), waves=4):
    """chain_runs on an all-long batch cut by length: run i is chained unless it heads its workgroup (i % waves == 0), is its
    stream's first run in the call, or is the one-frame last run of a stream whose last packet the EOS trim cut (`trimmed`)."""
    runs = by_length_runs(frames_per_stream, R)
    n = 0
    for i, (s, j, count) in enumerate(runs):
        last = i + 1 == len(runs) or runs[i + 1][0] != s
        if i % waves == 0 or j == 0 or (last and count == 1 and s in trimmed):
            continue
        n += 1
    return n


def all_long_packets(frames_per_stream, first_offset=0):
    """Stream-major all-long stereo packets (VPZ_PKT_NO_FLOOR), 2048 residue floats each, back to back from first_offset."""
    from vorbispizza_amd import make_packets
    counts = np.asarray(frames_per_stream, dtype=np.int64)
    pk = make_packets(int(counts.sum()))
    pk["stream"] = np.repeat(np.arange(len(counts)), counts)
    pk["flags"] = ALL_LONG | PKT_NO_FLOOR
    pk["granule"] = -1
    pk["residue_offset"] = first_offset + np.arange(len(pk), dtype=np.int64) * 2048
    return pk


def compare_all_long_with_oracle(orc, flags, granule, residue, pcm, chunk=2048, threads=4):
    """ONE all-long stereo stream against the oracle, every sample: flags / granule (numpy, per packet, stream order: the first
    packet primes the overlap), residue its spectra (a torch tensor, 2048 floats per packet, back to back) and pcm [2, samples]
    (torch) what the decoder wrote.  Chunk [a - 1, b) of the packets gives pcm[:, (a - 1) * 1024:(b - 1) * 1024] (a granule counts
    from the chunk's first output sample); the device data comes to the host one chunk at a time.  Returns (max |error|, RMS
    error, peak |oracle|, samples compared) and asserts that the sample counts agree."""
    import concurrent.futures as cf
    from vorbispizza_amd import make_packets
    n = len(flags)
    samples = int(pcm.shape[1])
    if n < 2:
        assert samples == 0
        return 0.0, 0.0, 0.0, 0
    edges = list(range(1, n, chunk)) + [n]

    def one(k):
        c0, b = edges[k] - 1, edges[k + 1]
        m = b - c0
        pk = make_packets(m)
        pk["flags"] = flags[c0:b]
        g = np.asarray(granule[c0:b], dtype=np.int64)
        pk["granule"] = np.where(g >= 0, g - c0 * 1024, -1)
        pk["residue_offset"] = np.arange(m, dtype=np.int64) * 2048
        fs = orc.FlooredStream(2, 256, 2048, pk, residue[c0 * 2048:b * 2048].cpu().numpy(), None, None)
        got = int(fs.run())
        if b < n:
            assert got == (m - 1) * 1024, (k, got)
        ref = fs.pcm[:, :got].astype(np.float64)
        gpu = pcm[:, c0 * 1024:c0 * 1024 + got].cpu().numpy().astype(np.float64)
        assert gpu.shape == ref.shape, (k, gpu.shape, ref.shape)
        d = np.abs(gpu - ref)
        return got, float(d.max(initial=0.0)), float((d * d).sum()), float(np.abs(ref).max(initial=0.0)), bool(np.isfinite(gpu).all())

    with cf.ThreadPoolExecutor(max_workers=threads) as ex:
        parts = list(ex.map(one, range(len(edges) - 1)))
    total = sum(p[0] for p in parts)
    assert total == samples, ("oracle samples", total, "decoder samples", samples)
    assert all(p[4] for p in parts), "NaN or Inf in the decoder's PCM"
    max_err = max(p[1] for p in parts)
    rms = (sum(p[2] for p in parts) / max(1, 2 * total)) ** 0.5
    return max_err, rms, max(p[3] for p in parts), total
