// P/Invoke binding of include/vorbispizza_pcm_pack.h -- windows of a device PCM array delivered as a dense, zero-padded batch in
// device memory.  A host that synthesises a batch into device memory (VorbisPizzaSynth.vpz_decoder_synth with MemDevice, interleaved)
// and hands the samples to a consumer on the same GPU fills one PackRow per window -- where it starts in the source array, how many
// samples it has, which row of the batch it becomes -- and makes one vpz_pcm_pack call: every named row gets its samples in the
// batch's layout ([rows][channels][frames] for the planar layouts, [rows][frames][channels] for the interleaved ones) and zeros
// behind them, asynchronously on the context's stream.  Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class GpuPcmPack
    {
        private const string Synth = "vorbispizza_synth";

        [StructLayout(LayoutKind.Sequential)]
        public struct PackRow                         // vpz_pack_row
        {
            public long Src;                          // element offset of the window's first sample (channel 0) in the source array
            public long Samples;                      // samples per channel to copy, 0..frames; the rest of the row becomes zero
            public long Row;                          // destination row, 0..dstRows-1
        }

        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_pcm_pack(IntPtr ctx, void* srcDev, long srcElems, int channels, int nRows, PackRow* rows, void* dstDev, long dstRows, long frames, int dstLayout);
    }
}
