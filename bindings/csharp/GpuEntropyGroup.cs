// P/Invoke binding of include/vorbispizza_entropy_group.h -- the entropy decode of Vorbis audio packets on the GPU for
// streams of DIFFERENT setup headers in one call.  A host that decodes a library groups its streams by channel count and
// block sizes, creates one group from the setup images of a class (GpuEntropyDecode.SetupImage), plans every stream
// (GpuEntropyDecode.vpzh_plan_range) with its index in the batch as the stream id, adds the mapping base of the stream's
// setup to its records and hands the whole batch to vpz_entropy_group_decode; vpz_decoder_synth (VorbisPizzaSynth.cs), on a
// decoder created from the union of the setups' floors and mappings, consumes the device-resident result on the same
// context without a synchronise.  Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class GpuEntropyGroup
    {
        private const string Synth = "vorbispizza_synth";

        public const int MaxSetups = 256;              // VPZ_ENTROPY_GROUP_MAX_SETUPS

        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_entropy_group_create(IntPtr ctx, void** images, ulong* sizes, int nSetups, out IntPtr group);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern void vpz_entropy_group_destroy(IntPtr group);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_entropy_group_decode(IntPtr group, int nStreams, byte* streamSetup, byte* streamMappingBase, long nPackets, void* packets, GpuEntropyDecode.Span* spans, byte* payload, long payloadBytes, int residueFormat, void* residue, long residueValues, short* posts, byte* postCounts, long nRecords, int memSpace);

        /// <summary>A group of the given setup images (one class: equal channels and block sizes); IntPtr.Zero when refused.</summary>
        public static IntPtr Create(IntPtr ctx, byte[][] images)
        {
            var handles = new GCHandle[images.Length];
            var ptrs = new void*[images.Length];
            var sizes = new ulong[images.Length];
            try
            {
                for (int i = 0; i < images.Length; i++)
                {
                    handles[i] = GCHandle.Alloc(images[i], GCHandleType.Pinned);
                    ptrs[i] = (void*)handles[i].AddrOfPinnedObject();
                    sizes[i] = (ulong)images[i].Length;
                }
                fixed (void** p = ptrs)
                fixed (ulong* s = sizes)
                    return vpz_entropy_group_create(ctx, p, s, images.Length, out IntPtr group) == 0 ? group : IntPtr.Zero;
            }
            finally
            {
                foreach (var h in handles)
                    if (h.IsAllocated) h.Free();
            }
        }
    }
}
