// P/Invoke binding of include/vorbispizza_entropy.h -- the entropy decode of Vorbis audio packets on the GPU -- and of
// the three entry points of include/vorbispizza_front.h that prepare it (eligibility, setup image, plan).  A host that
// decodes a library keeps the container and the setup headers on the CPU, plans each range of packets there and hands
// the payload to vpz_entropy_decode; vpz_decoder_synth (VorbisPizzaSynth.cs) consumes the device-resident result on the
// same context without a synchronise.  Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class GpuEntropyDecode
    {
        private const string Synth = "vorbispizza_synth", Host = "vorbispizza_host";

        public const int Version = 1;                  // VPZ_ENTROPY_VERSION
        public const uint ImageMagic = 0x45505A56;     // VPZ_ENTROPY_IMAGE_MAGIC
        public const int ImageVersion = 1;             // VPZ_ENTROPY_IMAGE_VERSION

        [StructLayout(LayoutKind.Sequential)]
        public struct Span                             // vpz_entropy_span
        {
            public long Offset;
            public long Size;
        }

        // ---- libvorbispizza_synth.so
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_entropy_version();
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_entropy_setup_create(IntPtr ctx, byte* image, ulong size, out IntPtr setup);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern void vpz_entropy_setup_destroy(IntPtr setup);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_entropy_decode(IntPtr setup, long nPackets, void* packets, Span* spans, byte* payload, long payloadBytes, int residueFormat, void* residue, long residueValues, short* posts, byte* postCounts, long nRecords, int memSpace);

        // ---- libvorbispizza_host.so
        [DllImport(Host, CallingConvention = CallingConvention.Cdecl)] public static extern int vpzh_gpu_decode_supported(IntPtr stream);
        [DllImport(Host, CallingConvention = CallingConvention.Cdecl)] public static extern int vpzh_get_entropy_setup(IntPtr stream, void* buf, ulong capacity, out ulong size);
        [DllImport(Host, CallingConvention = CallingConvention.Cdecl)] public static extern int vpzh_plan_range(IntPtr stream, long first, long count, int streamId, long residueBase, void* packets, Span* spans, byte* payload, long payloadCapacity, out long payloadUsed, out long residueUsed);

        /// <summary>The setup image of an opened stream (vpzh_open_memory), or null when the device cannot decode it.</summary>
        public static byte[] SetupImage(IntPtr stream)
        {
            if (vpzh_gpu_decode_supported(stream) == 0) return null;
            if (vpzh_get_entropy_setup(stream, null, 0, out ulong size) != 0) return null;
            var image = new byte[size];
            fixed (byte* p = image)
                if (vpzh_get_entropy_setup(stream, p, size, out size) != 0) return null;
            return image;
        }
    }
}
