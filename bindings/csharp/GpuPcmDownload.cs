// P/Invoke binding of include/vorbispizza_pcm.h -- a device-to-host copy that does not wait.  A host that synthesises a batch
// into device memory (VorbisPizzaSynth.vpz_decoder_synth with MemDevice) and wants a piece of every stream's area queues one
// vpz_pcm_download per piece and ends with one VorbisPizzaSynth.vpz_context_synchronize, where vpz_memcpy_d2h would wait for
// every copy.  Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class GpuPcmDownload
    {
        private const string Synth = "vorbispizza_synth";

        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_pcm_download(IntPtr ctx, void* hostDst, void* devSrc, ulong bytes);
    }
}
