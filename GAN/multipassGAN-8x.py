#!/usr/bin/env python3
"""8x progressive-growing training driver: the ``name value`` command line of the reference's
GAN/multipassGAN-8x.py (params :30-158) as example_run_training.py issues it for the first network
(upsamplingMode 2, upsampledData 0: low-res slices in, 8x slices out, three growing stages) and for the second /
third network (upsamplingMode 1 / 3, upsampledData 1: slices along the next axis, the previous network's output
volumes ``density_low_t%04d_2x2_%04d.uni`` / ``..._1x1_...`` as an extra high-res input channel, :231-238,:361-366).

What is rebuilt (reference line numbers): the data path :196-345 (FluidDataLoader slices of three
coherent frames with the add_adj_idcs neighbour channels, intermediate-resolution targets
``density_low_%i_%04d.uni`` for the 2x / 4x stages, ``density_high_%04d.uni`` for 8x), the growing schedule
:1885-1975 (stageIter iterations of fade-in + stageIter of stabilisation per stage, data re-loaded when a
stage completes), the iteration :1990-2060 (spatial critic, temporal critic on advected triples, generator)
through ``train.Trainer8x``, the polynomial learning-rate decay :995-1009 after 6 * stageIter iterations,
checkpoints ``model_%04d.ckpt.npz`` and the moving-average weights ``model_ema_%04d.ckpt.npz`` :1804-1812.

``out 1`` is the per-network output mode (see output_main).

``useVorticities 1`` (the tempoGAN vorticity input, addVorticity :1440-1446, called at :1482-1490,1508-1511): every
generator takes three more input channels behind all others (:350), computed from the velocity channels of each tile or
slice by ``mpgan_amd/vorticity.py`` -- the HIP kernel mpg_vorticity_append on device tiles, its numpy restatement on host
tiles (``deviceTiles 0``); in getinput before the 1-in-20 blanking, which scales the velocities and not the vorticity
(:1508-1532).  Deviations: (a) without ``useVelocities 1`` it is refused with a message (the reference widens the network
and feeds nothing); (b) ``out 1`` computes the channels on the low-res slice batch exactly as the network receives it
(the reference only counts them there, so a network trained with them cannot be run); (d) ``adv_mode 1 / 2`` and
``useVelInTDisc`` read the velocity as channels 1..3 of the 7-channel tile (the reference's 4-channel reshape, :1185,
fails there).

Not rebuilt: training with upsamplingMode 0 (``out 1`` runs it, see output_main; ``out 0`` says so and stops), flag /
k-eps inputs, PNG test images, TensorBoard.  ``lossScaling 1`` runs the dynamic loss scaling of :490-541 and every
stage uses its own optimisers over its own variable subset (:1305-1362) -- train.StagedAdam.
"""
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import mpgan_amd  # noqa: E402,F401
from mpgan_amd import checkpoint  # noqa: E402
from mpgan_amd import fluiddataloader as FDL  # noqa: E402
from mpgan_amd import paramhelpers as ph  # noqa: E402
from mpgan_amd import tilecreator_t as tc  # noqa: E402
from mpgan_amd import vorticity  # noqa: E402

P = {}
for name, default in [
        ("out", False), ("basePath", '../2ddata_gan/'), ("randSeed", 1), ("load_model_test", -1), ("load_model_no", -1),
        ("simSize", 64), ("tileSize", 16), ("upRes", 4), ("packedSimPath", '/data/share/GANdata/2ddata_sim/'),
        ("fromSim", 1000), ("toSim", -1), ("dataDim", 2), ("numOut", 200), ("saveOut", False), ("loadOut", -1),
        ("img", True), ("gif", False), ("ref", False), ("frame_min", 0), ("genModel", 'gen_test'),
        ("discModel", 'disc_test'), ("learningRate", 0.0002), ("decayLR", False), ("dropout", 1.0), ("dropoutOutput", 1.0),
        ("adam_beta1", 0.5), ("adam_beta2", 0.999), ("weight_dld", 1.0), ("lambda", 1.0), ("lambda2", 0.0),
        ("lambda_f", 1.0), ("lambda2_f", 1.0), ("lambda2_l1", 1.0), ("lambda2_l2", 1.0), ("lambda2_l3", 1.0),
        ("lambda2_l4", 1.0), ("useTempoD", True), ("useTempoL2", False), ("lambda_t", 1.0), ("lambda_t_l2", 0.0),
        ("batchSize", 128), ("batchSizeDisc", 128), ("batchSizeGen", 128), ("trainGAN", True),
        ("trainingIterations", 100000), ("discRuns", 1), ("genRuns", 1), ("batchNorm", False), ("pixelNorm", True),
        ("bnDecay", 0.999), ("useVelocities", 0), ("useVorticities", 0), ("useFlags", 0), ("useK_Eps_Turb", 0),
        ("premadeTiles", 0), ("dataAugmentation", 0), ("minScale", 0.85), ("maxScale", 1.15), ("rot", 2),
        ("transposeAxis", 0), ("minAngle", -90.0), ("maxAngle", 90.0), ("flip", 1), ("pretrain", 0), ("pretrainDisc", 0),
        ("pretrainGen", 0), ("testPathStartNo", 0), ("testInterval", 100), ("numTests", 128), ("outputInterval", 100),
        ("saveInterval", 200), ("alwaysSave", True), ("keepMax", 3), ("genTestImg", -1), ("note", ""),
        ("data_fraction", 0.3), ("frame_max", 200), ("adv_flag", True), ("adv_mode", 1), ("change_velocity", False),
        ("saveMetaData", 0), ("use_spatialdisc", True), ("velScale", 1.0), ("upsamplingMode", 2), ("upsampledData", False),
        ("genUni", False), ("upsampleFirst", True), ("usePixelShuffle", False), ("addBicubicUpsample", False),
        ("startingIter", 0), ("loadEmas", False), ("useVelInTDisc", False), ("upsampleMode", 1), ("lossScaling", False),
        ("stageIter", 25000), ("decayIter", 25000), ("maxFms", 256), ("use_wgan_gp", False), ("use_res_net", False),
        ("use_mb_stddev", False), ("deviceTiles", 1), ("use_LSGAN", False), ("startFms", 512), ("filterSize", 3), ("outNNTestNo", 17),
        ("firstNNArch", False), ("gDrop", False), ("add_adj_idcs", False), ("gpu", 2), ("synthWeights", 0), ("prec", "2"), ("trainPrec", "3"),
        ("uniCodec", 0), ("deviceLoader", 0), ("previews", 0), ("uniIndex", 0), ("deviceRead", 0)]:
    P[name] = ph.getParam(name, default)
ph.checkUnusedParams()


def fail(msg):
    print("ERROR: " + msg)
    exit(1)


useVorticities = int(P["useVorticities"]) > 0
if useVorticities and not int(P["useVelocities"]):
    fail("useVorticities 1 computes its channels from the velocity channels: useVelocities 1")


def output_main():
    """``out 1`` (generate3DUniForNewNetwork :1600-1780, output loop :2316-2324): ONE network per invocation, the
    volumes travel through .uni files as in the commented alternative of example_run_output.py:64-70:
      upsamplingMode 2, upsampledData 0 : first network          -> density_low_t%04d_2x2_%04d.uni   (t = load_model_test)
      upsamplingMode 1, upsampledData 1 : density_low_t<outNNTestNo>_2x2 in -> density_low_t%04d_1x1_%04d.uni
      upsamplingMode 3, upsampledData 1 : density_low_t<outNNTestNo>_1x1 in -> density_low_0x0_%04d.uni
    with the slicing axis given by transposeAxis (0..3) and the <5e-4 cutoff on every written volume; and the pair in
    which nothing is zoomed along z (:134,235-236,1614-1639,1711-1716,1763-1776):
      upsamplingMode 2, upsampledData 0, upsampleFirst 0 : first network on the simSize z slices
                                                           -> density_low_t%04d_2x2x1_%04d.uni (dimZ = simSize, :1763-1764)
      upsamplingMode 0, upsampledData 1 : density_low_t<outNNTestNo>_2x2x1 in, planes (y, z_low) along x, the network
                                          upsamples z itself -> density_low_t%04d_1x1x1_%04d.uni
    (multipass.plane_pass_8x / upsample_pass_8x, whose docstrings name the two places where the reference cannot run as
    written).  upsampleFirst 0 slices along z (transposeAxis 0); upsamplingMode 0 needs useVelocities 1 (the channel swap
    of :1637-1639 and the residual's channel 4) and has no vorticity channels, like the 4x driver.
    The shape of the low-res volume comes from the files ([Z, Y, X], any three sizes, for modes 2 / 1 / 3 and every
    transposeAxis): the generator is built for the plane of the pass (multipass.single_pass_plane_8x) and the written header
    carries the shape times upRes.  simSize is what the shape is expected to be (one line names the shape taken when it
    differs) and the cube size of training.  A non-cubic volume with previews 1, upsamplingMode 0 or upsampleFirst 0 exits
    with ERROR: and status 1 before a model is loaded."""
    from mpgan_amd import multipass, ops, uniio
    mode, upsampled = int(P["upsamplingMode"]), int(P["upsampledData"])
    up_first = int(P["upsampleFirst"]) > 0
    if (mode, upsampled) not in ((2, 0), (1, 1), (3, 1), (0, 1)) or int(P["dataDim"]) != 2:
        fail("output mode: upsamplingMode 2 (upsampledData 0) or 0 / 1 / 3 (upsampledData 1), dataDim 2")
    if not up_first and mode != 2:
        fail("upsampleFirst 0 belongs to the first network (upsamplingMode 2): the other modes read what it wrote")
    if int(P["useFlags"]) or int(P["useK_Eps_Turb"]):
        fail("flag / k-eps inputs are not supported")
    ta = int(P["transposeAxis"])
    if ta not in (0, 1, 2, 3):
        fail("transposeAxis %d (0..3)" % ta)
    if not up_first and ta != 0:
        fail("upsampleFirst 0 runs the network on the z slices as they are: transposeAxis 0")
    if mode == 0 and useVorticities:
        fail("upsamplingMode 0 has no vorticity channels (no training path produces such a network)")
    if mode == 0 and not int(P["useVelocities"]):
        fail("upsamplingMode 0 swaps and scales the velocity channels of its planes (:1636-1639) and takes its residual "
             "from channel 4 (:721): useVelocities 1")
    # extensions: uniIndex 1 = the written volumes record their unit sizes (device codecs), which lets deviceRead 1 = the
    # previous network's volume of each frame is read inside the frame loop and inflated on the GPU (uniio.readUniToDevice)
    uni_index, device_read = int(P["uniIndex"]), int(P["deviceRead"])
    if uni_index and not int(P["uniCodec"]):
        fail("uniIndex 1 needs the device codec (uniCodec 1 or 2)")
    up, sim = int(P["upRes"]), int(P["simSize"])
    base, sims = P["basePath"], P["packedSimPath"]
    from_sim, f0, f1 = int(P["fromSim"]), int(P["frame_min"]), int(P["frame_max"])
    vel = int(P["useVelocities"]) > 0
    n_ch = 4 if vel else 1
    first = mode == 2
    test_no, model_no = int(P["load_model_test"]), int(P["load_model_no"])
    mfl = ["density"] + (["velocity"] if vel else [])
    fl = FDL.FluidDataLoader(print_info=3, base_path=sims, base_path_y=sims, numpy_seed=int(P["randSeed"]),
                             filename="density_low_%04d.uni", filename_index_min=f0, oldNamingScheme=False, filename_y=None,
                             filename_index_max=f1, indices=[from_sim], data_fraction=1.0, multi_file_list=mfl,
                             multi_file_list_y=["density"])
    x_3d, _, _ = fl.get()
    x_3d[:, :, :, :, 1:4] = float(P["velScale"]) * x_3d[:, :, :, :, 1:4]                     # :361
    # the volume's shape comes from the files ([frame, Z, Y, X, C]); simSize is only what it is expected to be
    vol_shape = tuple(int(v) for v in x_3d.shape[1:4])
    if vol_shape != (sim,) * 3:
        print("simSize %d: the files hold %d x %d x %d (z, y, x) volumes, which is the shape taken" % ((sim,) + vol_shape))
    if not multipass.is_cube(vol_shape):
        for refused, why in ((int(P["previews"]), "previews 1 (the projections stack three sums of equal width)"),
                             (mode == 0, "upsamplingMode 0"), (not up_first, "upsampleFirst 0")):
            if refused:
                fail("%s takes cubic volumes, not %d x %d x %d" % ((why,) + vol_shape))
        tile_low = multipass.single_pass_plane_8x(vol_shape, ta)[0]
    else:
        tile_low = vol_shape[0]
    x_2 = None
    prev_name = {1: "density_low_t%04d_2x2", 0: "density_low_t%04d_2x2x1"}.get(mode, "density_low_t%04d_1x1") % int(
        P["outNNTestNo"]) + "_%04d.uni"                                                       # :231-238
    if upsampled and not device_read:
        fl2 = FDL.FluidDataLoader(print_info=0, base_path=sims, numpy_seed=int(P["randSeed"]), filename=prev_name,
                                  filename_index_min=f0, oldNamingScheme=False, filename_index_max=f1, indices=[from_sim],
                                  data_fraction=1.0, multi_file_list=["density"])
        x_2, _, _ = fl2.get()
    cfg = dict(tile_low=tile_low, up_res=up, channels=n_ch, first_gen=first, upsampling_mode=mode, filter_size=int(P["filterSize"]),
               start_fms=int(P["startFms"]), max_fms=int(P["maxFms"]), add_adj=int(P["add_adj_idcs"]) > 0 and first,
               first_nn_arch=int(P["firstNNArch"]) > 0 and first, use_res_net=int(P["use_res_net"]) > 0,
               pixel_norm=int(P["pixelNorm"]) > 0, batch_norm=int(P["batchNorm"]) > 0, upsample_mode=int(P["upsampleMode"]),
               add_bicubic=int(P["addBicubicUpsample"]) > 0, pixel_shuffle=int(P["usePixelShuffle"]) > 0 and first,
               vorticity=useVorticities)
    path = checkpoint.model_path(base, test_no, model_no, ema=int(P["loadEmas"]) > 0)
    try:
        params = checkpoint.load(path)
        print("Model restored from %s." % path)
    except FileNotFoundError as e:
        if not int(P["synthWeights"]):
            fail(str(e))
        params = None
        print("no checkpoint, seeded synthetic weights (synthWeights 1)")
    gen = multipass.Generator("growing_gen", cfg, params, prec=ops.parse_prec(P["prec"]), device="cuda:0",
                              seed=int(P["randSeed"]))
    out_name = {2: "density_low_t%04d_2x2" % test_no + ("" if up_first else "x1") + "_%04d.uni",
                1: "density_low_t%04d_1x1" % test_no + "_%04d.uni", 0: "density_low_t%04d_1x1x1" % test_no + "_%04d.uni",
                3: "density_low_0x0_%04d.uni"}[mode]                                          # :1768-1778
    print('*****OUTPUT ONLY*****')
    probe = sims + "sim_%04d/density_low_%04d.uni" % (from_sim, 0)
    head_0, _ = uniio.readUni(probe if os.path.exists(probe) else sims + "sim_%04d/density_low_%04d.uni" % (from_sim, f0))
    gen_uni = int(P["genUni"]) > 0
    previews = int(P["previews"])            # extension: 1 = source_%04d.png per frame into test_path (8x.py:1718)
    pictures = 0
    if previews:
        from mpgan_amd import preview
        os.makedirs(base + 'test_%04d/' % test_no, exist_ok=True)
        test_path, _ = ph.getNextGenericPath('out_%04d-%04d' % (test_no, model_no), 0, base + 'test_%04d/' % test_no)   # :428-429
    for layerno in range(f0, f1):
        print(layerno)
        t0 = time.time()
        low = torch.as_tensor(np.ascontiguousarray(x_3d[layerno - f0])).to("cuda:0")
        if upsampled and device_read:
            prev = uniio.readUniToDevice(os.path.join(sims, "sim_%04d/" % from_sim, prev_name % layerno), "cuda:0")[1][..., 0]
        else:
            prev = None if x_2 is None else torch.as_tensor(np.ascontiguousarray(x_2[layerno - f0][..., 0])).to("cuda:0")
        sink = preview.PreviewSink(test_path, layerno, int(P["tileSize"]) * up) if previews else None
        vol = multipass.single_pass_8x(gen, low, prev, up, ta, batch=2, apply_cutoff=gen_uni, previews=sink,
                                       upsample_first=up_first)
        torch.cuda.synchronize()
        if sink is not None:
            pictures += len(sink.written)
        print("time for network: {0:.6f}".format(time.time() - t0))
        if gen_uni:
            head = dict(head_0)
            head['dimZ'], head['dimY'], head['dimX'] = (n * up for n in vol_shape)
            if not up_first:
                head['dimZ'] = vol_shape[0]                                                           # :1763-1764
            uniio.writeUniFromDevice(sims + '/sim_%04d/' % from_sim + out_name % layerno, head, vol,
                                     codec={0: "host", 2: "device_dynamic"}.get(int(P["uniCodec"]), "device"),
                                     unit_index=bool(uni_index))
    print('Test finished, %d volumes written to %s.' % (f1 - f0, sims))
    if previews:
        print('%d pngs written to %s.' % (pictures, test_path))


if int(P["out"]) > 0:
    output_main()
    exit(0)
upsampling_mode, upsampled_data = int(P["upsamplingMode"]), int(P["upsampledData"])
if upsampling_mode == 0:
    fail("training upsamplingMode 0 is not built (the [tileSizeHigh, tileSizeLow] tiles of :298,378-382 and the faded "
         "heads of :729-737); the mode runs in output mode only: out 1 upsamplingMode 0 upsampledData 1")
if (upsampling_mode, upsampled_data) not in ((2, 0), (1, 1), (3, 1)) or int(P["dataDim"]) != 2:
    fail("training is implemented for the first network (upsamplingMode 2, upsampledData 0) and the second / third "
         "one (upsamplingMode 1 / 3, upsampledData 1), dataDim 2")
later_net = upsampling_mode != 2
if int(P["useFlags"]) or int(P["useK_Eps_Turb"]) or int(P["premadeTiles"]):
    fail("flag / k-eps inputs and premade tiles are not supported")
use_gdrop, useVelInTDisc = int(P["gDrop"]) > 0, int(P["useVelInTDisc"]) > 0
if use_gdrop and not int(P["use_LSGAN"]):
    fail("gDrop 1 needs use_LSGAN 1: the reference feeds the noise strengths only under use_LSGAN (:1993-2014)")
if useVelInTDisc and not (int(P["adv_flag"]) and int(P["useVelocities"]) and not int(P["add_adj_idcs"])):
    fail("useVelInTDisc 1 appends the velocity channels 1..3 of a 4-channel low-res tile (7 with vorticity) to the advected frames "
         "(:1185,1204-1208): adv_flag 1, useVelocities 1, add_adj_idcs 0")
upRes = int(P["upRes"])
if upRes != 8:
    fail("the growing networks are built for upRes 8")
kt, kt_l = float(P["lambda_t"]), float(P["lambda_t_l2"])
useTempoD = kt > 1e-6                                                # 8x.py:191-199
if kt_l > 1e-6:
    fail("the l2 temporal loss (lambda_t_l2) is not built; use lambda_t")
if useTempoD and int(P["adv_flag"]) and int(P["adv_mode"]) and not int(P["useVelocities"]):
    fail("adv_mode 1 / 2 (GAN.advect) advects with the velocity channels of the low-res tiles: useVelocities 1")

basePath, packedSimPath = P["basePath"], P["packedSimPath"]
simSizeLow, tileSizeLow = int(P["simSize"]), int(P["tileSize"])
fromSim, toSim = int(P["fromSim"]), int(P["toSim"])
toSim = fromSim if toSim == -1 else toSim
frame_min, frame_max = int(P["frame_min"]), int(P["frame_max"])
randSeed = int(P["randSeed"])
useVelocities, add_adj_idcs = int(P["useVelocities"]) > 0, int(P["add_adj_idcs"]) > 0
stageIter, decayIter, startingIter = int(P["stageIter"]), int(P["decayIter"]), int(P["startingIter"])
trainingIterations = stageIter * 6 + decayIter                      # :160-161
data_fraction, min_data_fraction = float(P["data_fraction"]), 0.08
batch = int(P["batchSize"])
aug = int(P["dataAugmentation"]) > 0
device = "cuda:0"
device_tiles = int(P["deviceTiles"]) > 0
if device_tiles:
    from mpgan_amd.tiles_device import DeviceTileCreator  # noqa: E402
# deviceLoader 1: the slice conversion of the training set (axis view, zoom, density filter, adjacent slices, row selection)
# runs in HIP kernels on the uploaded source and only the kept slices come back (fluiddataloader_device); 0 (default):
# the host FluidDataLoader
if int(P["deviceLoader"]) > 0:
    from mpgan_amd.fluiddataloader_device import DeviceFluidDataLoader  # noqa: E402

    def Loader(**kw):
        return DeviceFluidDataLoader(device=device, **kw)
else:
    Loader = FDL.FluidDataLoader

channelLayout_low, channelLayout_high, mfl, mfh = 'd', ('d,d' if later_net else 'd'), ["density"], ["density"]
if useVelocities:
    channelLayout_low += ',vx,vy,vz'
    mfl = mfl + ["velocity"]
if add_adj_idcs:
    channelLayout_low += ',d,d'
n_tileChannels = len(channelLayout_low.split(','))                  # of a tile as the tile creator cuts it
n_inputChannels = n_tileChannels + (vorticity.CHANNELS if useVorticities else 0)   # of the networks (:350)
if later_net and int(P["firstNNArch"]):
    fail("firstNNArch belongs to the first network")
# previous network's output volumes (:231-238) and the slicing axis of this pass (:301-307)
outNNTestNo = int(P["outNNTestNo"])
lowfilename_2 = {1: "density_low_t%04d_2x2" % outNNTestNo + "_%04d.uni", 3: "density_low_t%04d_1x1" % outNNTestNo + "_%04d.uni"}.get(upsampling_mode)
transpose_axis = {2: 0, 1: 2, 3: 1}[upsampling_mode]
dirIDs = np.linspace(fromSim, toSim, (toSim - fromSim + 1), dtype='int16')
mol = [o for o in range(3) for _ in mfl]
moh = [o for o in range(3) for _ in mfh]
stride = 3


def load_stage(currentUpres, first):
    """TileCreator + data of one growing stage (:290-345 at start-up, :1920-1960 at a stage change)"""
    tkw = dict(tileSizeLow=tileSizeLow, densityMinimum=0.002 if first else 0.01, channelLayout_high=channelLayout_high,
               simSizeLow=simSizeLow, dim=2, dim_t=3, channelLayout_low=channelLayout_low, upres=currentUpres, premadeTiles=False)
    # deviceTiles 1 (default): frames resident in HBM, batches cut / augmented by HIP kernels with the reference's random
    # decisions (tiles_device.DeviceTileCreator; tilecreator_t.py:457-546,1345-1414); 0: the host TileCreator
    tiCr = DeviceTileCreator(device=device, **tkw) if device_tiles else tc.TileCreator(**tkw)
    high = "density_high_%04d.uni" if currentUpres == upRes else "density_low_%i" % currentUpres + "_%04d.uni"
    off = 0 if first else stride * (int(round(math.log(currentUpres, 2))) - 1)
    common = dict(print_info=0, base_path=packedSimPath, base_path_y=packedSimPath, numpy_seed=randSeed,
                  add_adj_idcs=add_adj_idcs, conv_slices=True, conv_axis=transpose_axis,
                  select_random=(0.2 if later_net else 0.4) if first else 1.0, density_threshold=0.005 if first else 0.002,
                  axis_scaling_y=[1, 1, 1, 1], axis_scaling=[currentUpres, 1, 1, 1], filename="density_low_%04d.uni",
                  oldNamingScheme=False, filename_index_max=frame_max + off, filename_index_min=frame_min + off,
                  indices=dirIDs, multi_file_list_y=mfh * 3, multi_file_idxOff_y=moh)
    first_fraction = max(data_fraction * 2 / currentUpres, min_data_fraction)
    x_2 = None
    if later_net:      # the same slices of the previous network's output, read as the `y` of a density-only loader (:324-333)
        fl2 = Loader(filename_y=lowfilename_2, data_fraction=first_fraction, multi_file_list=["density"] * 3,
                     multi_file_idxOff=[0, 1, 2], **common)
    fl = Loader(filename_y=high, data_fraction=first_fraction if first else data_fraction, multi_file_list=mfl * 3,
                multi_file_idxOff=mol, **common)
    if aug:
        tiCr.initDataAugmentation(rot=int(P["rot"]), minScale=float(P["minScale"]), maxScale=float(P["maxScale"]),
                                  flip=int(P["flip"]))
    x, y, _ = fl.get()
    if later_net:
        _, x_2, _ = fl2.get()
    simSizeHigh = simSizeLow * upRes
    side_y = simSizeHigh if later_net else simSizeLow * currentUpres
    if tuple(x.shape[1:3]) != (simSizeLow, simSizeLow) or tuple(y.shape[1:3]) != (side_y, side_y):
        fail("training takes simSize cubes: simSize %d, the files hold slices of %s (input) and %s (target)"
             % (simSizeLow, tuple(x.shape[1:3]), tuple(y.shape[1:3])))
    if not later_net:
        x = x.reshape(-1, 1, simSizeLow, simSizeLow, n_tileChannels * 3)
        y = y.reshape(-1, 1, simSizeLow * currentUpres, simSizeLow * currentUpres, 3)
    else:
        # (:372-376) per frame the pair (target, previous pass): the reference's reshape / concatenate / reshape of
        # the three-frame arrays is this interleave of their last axes
        x = x.reshape(-1, 1, simSizeLow, simSizeLow, n_tileChannels * 3)
        y = y.reshape(-1, 1, simSizeHigh, simSizeHigh, 3)
        x_2 = x_2.reshape(-1, 1, simSizeHigh, simSizeHigh, 3)
        y = np.stack((y, x_2), axis=-1).reshape(-1, 1, simSizeHigh, simSizeHigh, 6)
    tiCr.addData(x, y)
    return tiCr


currentUpres = 8 if later_net else min(2 ** (startingIter // (stageIter * 2) + 1), 8)   # :213-217
tiCr = load_stage(currentUpres, True)
print("Random seed: {}".format(randSeed))
np.random.seed(randSeed)
test_path, _ = ph.getNextTestPath(int(P["testPathStartNo"]), basePath)
print("\nUsing parameters:\n" + ph.paramsToString())
ph.writeParams(test_path + "params.json")

from mpgan_amd import heldout, ops  # noqa: E402
from mpgan_amd.arch import Cfg8x  # noqa: E402
from mpgan_amd.train import Trainer8x, gdrop_schedule  # noqa: E402

cfg = Cfg8x(tileSizeLow=tileSizeLow, upRes=upRes, n_inputChannels=n_inputChannels, upsampling_mode=upsampling_mode,
            upsampleMode=int(P["upsampleMode"]), filterSize=int(P["filterSize"]), start_fms=int(P["startFms"]),
            max_fms=int(P["maxFms"]), first_nn_arch=int(P["firstNNArch"]) > 0, use_res_net=int(P["use_res_net"]) > 0,
            pixel_norm=int(P["pixelNorm"]) > 0, addBicubicUpsample=int(P["addBicubicUpsample"]) > 0,
            use_mb_stddev=int(P["use_mb_stddev"]) > 0, bn_decay=float(P["bnDecay"]),
            usePixelShuffle=int(P["usePixelShuffle"]) > 0,        # read by the first network only (growBlockGen)
            useVelInTDisc=useVelInTDisc and useTempoD, gDrop=use_gdrop)
learning_rate = float(P["learningRate"])
trainer = Trainer8x(cfg, device=device, learning_rate=learning_rate, beta1=float(P["adam_beta1"]),
                    beta2=float(P["adam_beta2"]), lambda_l1=float(P["lambda"]), lambda2=float(P["lambda2"]),
                    weight_dld=float(P["weight_dld"]), use_wgan_gp=int(P["use_wgan_gp"]) > 0,
                    use_LSGAN=int(P["use_LSGAN"]) > 0, seed=randSeed, use_tempo=useTempoD, lambda_t=kt,
                    adv_flag=int(P["adv_flag"]) > 0, loss_scaling=int(P["lossScaling"]) > 0,
                    adv_mode=int(P["adv_mode"]), batch_norm=int(P["batchNorm"]) > 0, prec=ops.parse_prec(P["trainPrec"]))
if int(P["load_model_test"]) >= 0:
    params = checkpoint.load(checkpoint.model_path(basePath, int(P["load_model_test"]), int(P["load_model_no"])))
    with torch.no_grad():
        for n_, t_ in trainer.sess.params.items():
            if n_ in params:
                t_.copy_(torch.as_tensor(params[n_], device=t_.device))
    n_slots = trainer.load_slot_state(params)                         # the Saver restores the optimiser slots too
    print("Model restored (%d optimiser slot pairs)." % n_slots)


def widen(bx):
    """addVorticity (:1440-1446): the three vorticity channels behind every tile's own, computed where the tiles live"""
    return vorticity.append(bx.reshape(-1, 1, tileSizeLow, tileSizeLow, n_tileChannels)) if useVorticities else bx


def getinput(size=batch, isTraining=True, augment=aug):
    """:1497-1537 incl. the 1-in-20 empty-density batches"""
    if device_tiles:
        batch_xs, batch_ys = tiCr.selectRandomTilesDevice(size, isTraining, augment=augment)
    else:
        batch_xs, batch_ys = tiCr.selectRandomTiles(selectionSize=size, isTraining=isTraining, augment=augment)
    batch_xs = widen(batch_xs)                                       # :1508-1511, before the blanking
    if not min(np.random.randint(0, 20), 1):
        batch_xs[:, :, :, :, 0:1] = 0
        if add_adj_idcs:
            batch_xs[:, :, :, :, 4:6] = 0
        batch_xs[:, :, :, :, 1:4] *= (1.0 + np.random.rand() * 1.5)
        batch_ys[:, :, :, :, :] = 0
    return batch_xs.reshape(-1, cfg.n_input), batch_ys.reshape(size, -1)


def getTempoinput(size=batch, isTraining=True, augment=aug):
    if device_tiles:
        bx, by, bp = tiCr.selectRandomTempoTilesDevice(size, isTraining, augment, 3, 0.5)
    else:
        bx, by, bp = tiCr.selectRandomTempoTiles(size, isTraining, augment, 3, 0.5)
    n = bx.shape[0]
    return widen(bx).reshape(n, -1), by.reshape(n, -1), bp.reshape(n, -1)    # :1482-1490


save_no = 0


def saveModel():
    global save_no
    trainer.sess.sync_to_store()
    allp = trainer.sess.vars.numpy()
    full = dict(allp)
    full.update(trainer.slot_state())
    checkpoint.save(test_path + 'model_%04d.ckpt' % save_no, full)
    ema = dict(allp)
    for n_, e_ in zip(trainer.opt_g.names, trainer.ema):           # MovingAverageOptimizer.swapping_saver (:1366)
        ema[n_] = e_.detach().cpu().numpy()
    checkpoint.save(test_path + 'model_ema_%04d.ckpt' % save_no, ema)
    print('Saved Model %04d.' % save_no)
    save_no += 1


def poly_decay(step):
    """tf.train.polynomial_decay(lr, step, decayIter, lr * 0.05, power=1.1) (:1006-1009)"""
    s = min(step, decayIter)
    return (learning_rate - learning_rate * 0.05) * (1 - s / float(decayIter)) ** 1.1 + learning_rate * 0.05


# growing schedule (:1885-1975)
interpolate_Perc = True
start_interpol = stageIter * int(math.floor(startingIter // (stageIter * 2))) * 2 + stageIter
interpol_c = int(math.floor(startingIter // (stageIter * 2)) * stageIter)
if (startingIter // stageIter) % 2 == 0:
    interpol_c += (startingIter - interpol_c) % stageIter
    interpol_c += stageIter
else:
    interpolate_Perc = False
lrgs = 0
discRuns, genRuns = int(P["discRuns"]), int(P["genRuns"])
outputInterval, saveInterval = int(P["outputInterval"]), int(P["saveInterval"])
decayLR = int(P["decayLR"]) > 0
# the "test model" section (:2094-2196): every testInterval iterations numTests tiles of the train and of the test split go
# through the networks with `train: False` at the current blending percentage (Trainer8x.evaluate); genTestImg > -1
# writes the sampler's image of the first frame with every report (:2263-2266)
testInterval, numTests, genTestImg = int(P["testInterval"]), int(P["numTests"]), int(P["genTestImg"])


noticed = False


def test_split(tiles):
    """does the stage's tile creator hold test frames?  The first one without says so, once per run"""
    global noticed
    have = tiles.setBorders[1] > tiles.setBorders[0]
    if not have and not noticed:
        noticed = True
        print('no test frames in the data (%d frames): the test section is skipped' % tiles.setBorders[2])
    return have


have_test = test_split(tiCr)
log, image_no = heldout.HeldOutLog(), 0
# gDrop (:1878-1882): noise strengths of the two critics and the running scores they follow, all 0 at the start
gdrop_strength_d = gdrop_strength_t = 0.0
d_fakeScores_train = t_fakeScores_train = 0.0
t0 = time.time()
print('\n*****TRAINING STARTED***** (stop with ctrl-c)\n')
for it in range(startingIter, trainingIterations):
    if it - start_interpol == 0:
        interpolate_Perc = False
    if it - start_interpol == stageIter and currentUpres < upRes:    # a stage is complete: next resolution, new data
        saveModel()
        currentUpres *= 2
        start_interpol = it + stageIter
        interpolate_Perc = True
        tiCr = load_stage(currentUpres, False)
        have_test = test_split(tiCr)
        print("--------------------------NEW UPRES: %d--------------------------" % currentUpres)
    if interpolate_Perc:
        interpol_c += 1
        currBlendPer = interpol_c / stageIter
    else:
        currBlendPer = int(round(interpol_c / stageIter))
    currBlendPer = min(max(currBlendPer, 1.0), 3.0)
    if it >= stageIter * 6 and decayLR:
        lrgs += 1
    lr = poly_decay(lrgs) if decayLR else learning_rate
    for opt in [trainer.opt_d, trainer.opt_g] + ([trainer.opt_t] if useTempoD else []):
        opt.lr = lr
    index = int(round(math.log(currentUpres, 2)) - 1)               # the growing stage's optimisers (:1978)
    for _ in range(discRuns):
        bx, by = getinput()
        log.add_train("avgCost_disc", trainer.disc_step(bx, by, currBlendPer, stage=index,
                                                         gdrop_str_d=gdrop_strength_d)["disc_loss"].detach())
    tempo = None
    if useTempoD:
        for _ in range(discRuns):
            tempo = getTempoinput()
            Lt = trainer.tempo_disc_step(tempo[0], tempo[1], tempo[2], currBlendPer, stage=index, gdrop_str_t=gdrop_strength_t)
            log.add_train("avgTemCost_disc", Lt["t_disc_loss"].detach())
    gdrop_strength_d = gdrop_strength_t = 0.0                        # :2013-2014: the generator step is fed 0
    for _ in range(genRuns):
        bx, by = getinput()
        if useTempoD:
            tempo = getTempoinput()
        L = trainer.gen_step(bx, by, currBlendPer, tempo, stage=index, gdrop_str_d=gdrop_strength_d,
                             gdrop_str_t=gdrop_strength_t)
        log.add_train("avgCost_gen", L["g_loss_d"].detach())
        log.add_train("avgL1Cost_gen", L["l1_loss"].detach())
        if useTempoD:
            log.add_train("avgTemCost_gen", L["g_loss_t"].detach())
    if use_gdrop:                                                    # :2086-2092 (check_gdrop_interval 1; LSGAN only)
        d_fakeScores_train, gdrop_strength_d = gdrop_schedule(d_fakeScores_train, float(L["d_sig_g"]))
        if useTempoD:
            t_fakeScores_train, gdrop_strength_t = gdrop_schedule(t_fakeScores_train, float(L["t_sig_g"]))
    test_now, print_now, image_now = heldout.schedule(it, testInterval, outputInterval, genTestImg, have_test)
    if test_now:                                                     # draw order of :2099-2137
        train_b, test_b = getinput(numTests, True, False), getinput(numTests, False, False)
        tempo_b = tempo_test_b = None
        if useTempoD:
            tempo_b, tempo_test_b = getTempoinput(numTests, True, False), getTempoinput(numTests, False, False)
        log.add_test(trainer.evaluate(train_b[0], train_b[1], test_b[0], test_b[1], tempo=tempo_b, tempo_test=tempo_test_b,
                                      percentage=currBlendPer, stage=index, gdrop_str_d=gdrop_strength_d,
                                      gdrop_str_t=gdrop_strength_t))
    if print_now:
        print(log.report(it, trainingIterations, outputInterval, discRuns, genRuns, k=trainer.k, kt=kt, kt_l=kt_l,
                         blend=currBlendPer))
        print('\t{} iterations took {:.2f} seconds.'.format(outputInterval, time.time() - t0))
        if use_gdrop:
            print('\tgdrop_strength_d: {:.6f}, gdrop_strength_t: {:.6f}'.format(gdrop_strength_d, gdrop_strength_t))
        if image_now:
            trainer.sample_frame_image(tiCr, heldout.frame_index(fromSim, fromSim, frame_max), test_path + 'test_img/',
                                       image_no, simSizeLow * upRes, percentage=currBlendPer, use_vorticity=useVorticities)
            image_no += 1
        t0 = time.time()
    if (it + 1) % saveInterval == 0:
        saveModel()
saveModel()
print('\n*****TRAINING FINISHED*****')
print('Test path: %s' % test_path)
