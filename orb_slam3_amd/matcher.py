"""Host-side mirror of ORB_SLAM3::ORBmatcher (/root/reference/include/ORBmatcher.h:36-103) over the C ABI.

The reference matchers walk Frame / KeyFrame / MapPoint pointer graphs; at this boundary those are passed
flattened (numpy arrays).  `FrameView` carries what the matchers read of a Frame: undistorted keypoints,
descriptors, image bounds (for the 64x48 grid) and the per-level scale factors.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import KP_DTYPE, BowKeyFrame, FeatVec, FrameDesc, FuseQueries, KeyFrameGate, KeyFrameKb8Gate, NewPointsParams, NewPointsStereo, NewPointsView, PAIR_PREDICATE, PinholeGate, check, ptr


@dataclass
class FrameView:
    keypoints_un: np.ndarray          # KP_DTYPE [N]   (Frame::mvKeysUn)
    descriptors: np.ndarray           # uint8 [N,32]   (Frame::mDescriptors)
    min_x: float
    max_x: float
    min_y: float
    max_y: float
    scale_factors: np.ndarray         # float32 [nlevels] (Frame::mvScaleFactors)
    u_right: np.ndarray | None = None  # float32 [N] (Frame::mvuRight) or None for mono

    def c_struct(self):
        self.keypoints_un = np.ascontiguousarray(self.keypoints_un, KP_DTYPE)
        self.descriptors = np.ascontiguousarray(self.descriptors, np.uint8)
        self.scale_factors = np.ascontiguousarray(self.scale_factors, np.float32)
        if self.u_right is not None:
            self.u_right = np.ascontiguousarray(self.u_right, np.float32)
        return FrameDesc(self.keypoints_un.ctypes.data, self.descriptors.ctypes.data, len(self.keypoints_un),
                         self.min_x, self.max_x, self.min_y, self.max_y, self.scale_factors.ctypes.data,
                         len(self.scale_factors), None if self.u_right is None else self.u_right.ctypes.data)


@dataclass
class FisheyeRig:
    """What Frame::ComputeStereoFishEyeMatches reads of a KannalaBrandt8 stereo rig (orbx_kb8_rig)."""
    cam_left: np.ndarray              # float32 [8] mpCamera->mvParameters (fx, fy, cx, cy, k0..k3)
    cam_right: np.ndarray             # float32 [8] mpCamera2->mvParameters
    R_lr: np.ndarray                  # float32 [3, 3] Frame::mRlr
    t_lr: np.ndarray                  # float32 [3] Frame::mtlr


class FeatureVector:
    """DBoW2::FeatureVector as arrays: `nodes` ascending node ids, `lists[k]` = feature indices of node k."""

    def __init__(self, nodes, lists):
        self.node_id = np.ascontiguousarray(nodes, np.uint32)
        assert np.all(np.diff(self.node_id.astype(np.int64)) > 0), "node ids must be strictly ascending (std::map order)"
        self.node_ptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
        self.index = (np.concatenate(lists) if len(lists) else np.zeros(0)).astype(np.int32)

    @classmethod
    def from_node_of_feature(cls, node_of_feature):
        """Build from a per-feature node id array (features listed in ascending index inside a node, as
        TemplatedVocabulary::transform / FeatureVector::addFeature produce)."""
        node_of_feature = np.asarray(node_of_feature)
        nodes = np.unique(node_of_feature)
        return cls(nodes, [np.nonzero(node_of_feature == nd)[0] for nd in nodes])

    def c_struct(self, cls=FeatVec):
        return cls(self.node_id.ctypes.data, self.node_ptr.ctypes.data, self.index.ctypes.data, len(self.node_id))


class DeviceFrame:
    """A frame resident on the device across matcher calls (orbx_frame, include/orbx.h): what Frame::ExtractORB / UndistortKeyPoints /
    AssignFeaturesToGrid build once per frame -- keypoints, descriptors, optional mvuRight, the count, the scale factors and the 64x48 grid.
    It belongs to the matcher it was created with; ORBmatcher.SearchByProjection / SearchByProjectionFrame / SearchLocalPoints take it in
    place of a FrameView."""

    def __init__(self, matcher: "ORBmatcher", cap: int):
        self._L = _lib.lib()
        self.matcher = matcher        # (the owner outlives the handle)
        self.cap = int(cap)
        self._h = C.c_void_p()
        check(self._L.orbx_frame_create(matcher._h, self.cap, C.byref(self._h)), "orbx_frame_create")
        matcher._frames[self._h.value] = self._h   # (the owner destroys what is left of its handles before itself: ORBmatcher.__del__)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and self.matcher._frames.pop(h.value, None) is not None:
            self._L.orbx_frame_destroy(h)
        self._h = None

    def load(self, F: "FrameView"):
        """Upload a host frame once and build its grid (orbx_frame_load_host)."""
        fd = F.c_struct()
        check(self._L.orbx_frame_load_host(self._h, C.byref(fd)), "orbx_frame_load_host")   # (the rows are staged before it returns)
        return self

    def load_batch(self, extractor, f: int, bounds=None, scale_factors=None):
        """Frame f of the extractor's last batch, copied on the device (orbx_frame_load_batch): asynchronous, no host synchronisation.
        bounds = (minX, maxX, minY, maxY) or None (the extractor's camera / image rectangle); scale_factors None = the extractor's."""
        b, sf = _f32(bounds), _f32(scale_factors)
        check(self._L.orbx_frame_load_batch(self._h, extractor._h, int(f), ptr(b), ptr(sf), 0 if sf is None else len(sf)), "orbx_frame_load_batch")
        return self

    def load_stereo_batch(self, extractor, f: int, bounds=None, scale_factors=None):
        """load_batch plus the frame's mvuRight, mvDepth and raw key points from the (left) extractor's last stereo_device / rgbd_device stage, copied
        on the device in the same launch (orbx_frame_load_stereo_batch).  Refused when no stage has run on the extractor's current batch."""
        b, sf = _f32(bounds), _f32(scale_factors)
        check(self._L.orbx_frame_load_stereo_batch(self._h, extractor._h, int(f), ptr(b), ptr(sf), 0 if sf is None else len(sf)),
              "orbx_frame_load_stereo_batch")
        return self

    def load_host_stereo(self, F: "FrameView", depth, keys_xy=None):
        """load with mvuRight (F.u_right) required, and mvDepth [n] / the raw mvKeys[i].pt [n, 2] (None: the undistorted points) in the same upload
        (orbx_frame_load_host_stereo)."""
        fd = F.c_struct()
        d, xy = _f32(depth), _f32(keys_xy)
        assert len(d) == fd.n and (xy is None or xy.shape == (fd.n, 2))
        check(self._L.orbx_frame_load_host_stereo(self._h, C.byref(fd), ptr(d), ptr(xy)), "orbx_frame_load_host_stereo")   # (staged before it returns)
        return self

    def count(self) -> int:
        n = C.c_int(0)
        check(self._L.orbx_frame_count(self._h, C.byref(n)), "orbx_frame_count")
        return n.value

    def load_fisheye(self, left: "FrameView", kps_right, l2r, r2l):
        """Upload a fisheye-stereo frame (orbx_frame_load_host_fisheye): left.keypoints_un = mvKeys, left.descriptors = ALL N rows,
        kps_right = mvKeysRight, l2r / r2l = mvLeftToRightMatch / mvRightToLeftMatch."""
        self._kr = np.ascontiguousarray(kps_right, KP_DTYPE)
        self._l2r, self._r2l = _i32(l2r), _i32(r2l)
        fd = left.c_struct()
        check(self._L.orbx_frame_load_host_fisheye(self._h, C.byref(fd), ptr(self._kr), len(self._kr), ptr(self._l2r), ptr(self._r2l)),
              "orbx_frame_load_host_fisheye")
        return self

    def load_stereo_fisheye_batch(self, left_ex, right_ex, f: int, bounds=None, scale_factors=None):
        """Frame f of the last ORBextractor.stereo_fisheye_device stage, copied on the device (orbx_frame_load_stereo_fisheye_batch): asynchronous;
        the counts stay on the device until the first search.  bounds / scale_factors as load_batch."""
        b, sf = _f32(bounds), _f32(scale_factors)
        check(self._L.orbx_frame_load_stereo_fisheye_batch(self._h, left_ex._h, right_ex._h, int(f), ptr(b), ptr(sf), 0 if sf is None else len(sf)),
              "orbx_frame_load_stereo_fisheye_batch")
        return self

    def counts(self):
        """(N_left, N_right); N_right = -1 for a monocular / rectified frame (Frame::Nleft == -1)."""
        nl, nr = C.c_int(0), C.c_int(0)
        check(self._L.orbx_frame_counts(self._h, C.byref(nl), C.byref(nr)), "orbx_frame_counts")
        return nl.value, nr.value

    def compute_bow(self, voc: "ORBVocabulary", levelsup: int = 4, download: bool = True):
        """Frame::ComputeBoW's transform on the resident descriptors (orbx_frame_compute_bow); the FeatureVector stays in the handle for
        ORBmatcher.SearchByBoWDevice.  download=True returns (word_id[N], node_id[N]); download=False returns None and does not wait."""
        if not download:
            check(self._L.orbx_frame_compute_bow(self.matcher._h, self._h, voc._h, int(levelsup), None, None), "orbx_frame_compute_bow")
            return None
        w = np.zeros(self.cap, np.int32)
        nd = np.zeros(self.cap, np.int32)
        check(self._L.orbx_frame_compute_bow(self.matcher._h, self._h, voc._h, int(levelsup), ptr(w), ptr(nd)), "orbx_frame_compute_bow")
        n = self.count()   # (known after the call: no further synchronisation)
        return w[:n], nd[:n]

    def compute_bow_fisheye(self, voc: "ORBVocabulary", levelsup: int = 4, download: bool = True):
        """compute_bow for a fisheye-stereo handle (orbx_frame_compute_bow_fisheye): all N = N_left + N_right rows are transformed; the
        FeatureVector stays in the handle for ORBmatcher.SearchByBoWDeviceFisheye.  download=True returns (word_id[N], node_id[N]) in the rig's
        numbering (features >= N_left are the right camera's); download=False returns None and does not wait."""
        if not download:
            check(self._L.orbx_frame_compute_bow_fisheye(self.matcher._h, self._h, voc._h, int(levelsup), None, None), "orbx_frame_compute_bow_fisheye")
            return None
        w = np.zeros(self.cap, np.int32)
        nd = np.zeros(self.cap, np.int32)
        check(self._L.orbx_frame_compute_bow_fisheye(self.matcher._h, self._h, voc._h, int(levelsup), ptr(w), ptr(nd)), "orbx_frame_compute_bow_fisheye")
        n = self.count()   # (known after the call: no further synchronisation)
        return w[:n], nd[:n]

    def bow_vector(self):
        """Frame::mBowVec after compute_bow / compute_bow_fisheye (orbx_frame_bow_vector): (word_id ascending, value normalised), tf-idf and L1 as
        TemplatedVocabulary::transform makes it, built on the device from the kept word ids.  One synchronisation."""
        w, v, n = np.zeros(max(self.cap, 1), np.int32), np.zeros(max(self.cap, 1), np.float64), C.c_int(0)
        check(self._L.orbx_frame_bow_vector(self.matcher._h, self._h, ptr(w), ptr(v), C.byref(n)), "orbx_frame_bow_vector")
        return w[:n.value], v[:n.value]


class DeviceKeyFrame:
    """An immutable key frame resident on the device (orbx_keyframe, include/orbx.h): what KeyFrame::KeyFrame(Frame&) copies of the frame --
    mvKeysUn, descriptors, optional mvuRight, scale factors, mvInvLevelSigma2, the bounds and the 64x48 grid.  It belongs to no matcher: every
    ORBmatcher of the same device may search it (FuseSearchKeyFrames / FuseMapPoints), from any thread.  close() (or garbage collection) frees it;
    no call that was handed the key frame may be running then.
    A fisheye-stereo key frame (from_frame_fisheye / from_host_fisheye) holds mvKeys, mvKeysRight, all N descriptor rows, both counts and a grid per
    camera; FuseSearchKeyFramesFisheye / FuseMapPointsFisheye search it, compute_bow_fisheye / bow_from_frame_fisheye attach its BoW for
    ORBmatcher.SearchByBoWResidentFisheye / SearchByBoWKeyFramesResidentFisheye / SearchForTriangulationResidentKB8; the calls of the
    monocular kind refuse it."""

    def __init__(self, handle):
        self._L = _lib.lib()
        self._h = handle

    @classmethod
    def from_frame(cls, matcher: "ORBmatcher", frame: "DeviceFrame", inv_level_sigma2=None) -> "DeviceKeyFrame":
        """Device-to-device copy of a loaded monocular / rectified DeviceFrame of `matcher` (orbx_keyframe_from_frame): asynchronous, the
        frame may be reloaded right away."""
        isg = _f32(inv_level_sigma2)
        h = C.c_void_p()
        check(_lib.lib().orbx_keyframe_from_frame(matcher._h, frame._h, ptr(isg), C.byref(h)), "orbx_keyframe_from_frame")
        return cls(h)

    @classmethod
    def from_host(cls, matcher: "ORBmatcher", F: "FrameView", inv_level_sigma2=None) -> "DeviceKeyFrame":
        """The same object from host arrays (orbx_keyframe_create_host): one upload, the grid built as FuseSearch builds it."""
        isg = _f32(inv_level_sigma2)
        fd = F.c_struct()
        h = C.c_void_p()
        check(_lib.lib().orbx_keyframe_create_host(matcher._h, C.byref(fd), ptr(isg), C.byref(h)), "orbx_keyframe_create_host")   # (staged before it returns)
        return cls(h)

    @classmethod
    def create_host_stereo(cls, matcher: "ORBmatcher", F: "FrameView", depth, keys_xy=None, inv_level_sigma2=None) -> "DeviceKeyFrame":
        """from_host with mvuRight (F.u_right) required, mvDepth [n] and the raw mvKeys[i].pt [n, 2] (None: the undistorted points) in the same
        upload (orbx_keyframe_create_host_stereo): the key frame the `_stereo` forms of CreateNewMapPoints' triangulation decide stereo pairs on.
        from_frame of a DeviceFrame loaded with load_stereo_batch / load_host_stereo gives the same object."""
        isg, d, xy = _f32(inv_level_sigma2), _f32(depth), _f32(keys_xy)
        fd = F.c_struct()
        assert len(d) == fd.n and (xy is None or xy.shape == (fd.n, 2))
        h = C.c_void_p()
        check(_lib.lib().orbx_keyframe_create_host_stereo(matcher._h, C.byref(fd), ptr(d), ptr(xy), ptr(isg), C.byref(h)),
              "orbx_keyframe_create_host_stereo")   # (staged before it returns)
        return cls(h)

    @classmethod
    def from_frame_fisheye(cls, matcher: "ORBmatcher", frame: "DeviceFrame", inv_level_sigma2=None) -> "DeviceKeyFrame":
        """Device-to-device copy of a loaded fisheye-stereo DeviceFrame of `matcher` (orbx_keyframe_from_frame_fisheye): both cameras' rows, both
        counts and both grids; asynchronous, also while the counts are still on the device; the frame may be reloaded right away."""
        isg = _f32(inv_level_sigma2)
        h = C.c_void_p()
        check(_lib.lib().orbx_keyframe_from_frame_fisheye(matcher._h, frame._h, ptr(isg), C.byref(h)), "orbx_keyframe_from_frame_fisheye")
        return cls(h)

    @classmethod
    def from_host_fisheye(cls, matcher: "ORBmatcher", left: "FrameView", kps_right, inv_level_sigma2=None) -> "DeviceKeyFrame":
        """A fisheye-stereo key frame from host arrays (orbx_keyframe_create_host_fisheye): left.keypoints_un = mvKeys, left.descriptors = ALL
        N_left + N_right rows, kps_right = mvKeysRight.  One upload, a grid per camera."""
        isg = _f32(inv_level_sigma2)
        kr = np.ascontiguousarray(kps_right, KP_DTYPE)
        fd = left.c_struct()
        h = C.c_void_p()
        check(_lib.lib().orbx_keyframe_create_host_fisheye(matcher._h, C.byref(fd), ptr(kr), len(kr), ptr(isg), C.byref(h)),
              "orbx_keyframe_create_host_fisheye")   # (staged before it returns)
        return cls(h)

    def count(self) -> int:
        n = C.c_int(0)
        check(self._L.orbx_keyframe_count(self._h, C.byref(n)), "orbx_keyframe_count")
        return n.value

    def counts(self):
        """(N_left, N_right); N_right = -1 for a monocular / rectified key frame (orbx_keyframe_counts)."""
        nl, nr = C.c_int(0), C.c_int(0)
        check(self._L.orbx_keyframe_counts(self._h, C.byref(nl), C.byref(nr)), "orbx_keyframe_counts")
        return nl.value, nr.value

    def compute_bow(self, matcher: "ORBmatcher", voc: "ORBVocabulary", levelsup: int = 4, download: bool = True, cap: int | None = None,
                    fn: str = "orbx_keyframe_compute_bow"):
        """KeyFrame::ComputeBoW on the resident descriptors (orbx_keyframe_compute_bow): the key frame keeps its FeatureVector for
        ORBmatcher.SearchByBoWResident / SearchByBoWKeyFramesResident / SearchForTriangulationResident.  Set once: a second call with the same
        vocabulary and levelsup only returns the ids.  download=True returns (word_id[N], node_id[N]); download=False returns None and does not
        wait.  cap: the size of the id buffers while N is on the device only (the capacity of the frame handle the key frame was made from);
        None = count first."""
        self._voc = voc   # (the vocabulary outlives the key frame's BoW state)
        if not download:
            check(getattr(self._L, fn)(matcher._h, self._h, voc._h, int(levelsup), None, None), fn)
            return None
        size = self.count() if cap is None else int(cap)
        w, nd = np.zeros(max(size, 1), np.int32), np.zeros(max(size, 1), np.int32)
        check(getattr(self._L, fn)(matcher._h, self._h, voc._h, int(levelsup), ptr(w), ptr(nd)), fn)
        n = self.count()   # (known after the call: no further synchronisation)
        return w[:n], nd[:n]

    def compute_bow_fisheye(self, matcher: "ORBmatcher", voc: "ORBVocabulary", levelsup: int = 4, download: bool = True, cap: int | None = None):
        """compute_bow for a fisheye-stereo key frame (orbx_keyframe_compute_bow_fisheye): all N = N_left + N_right descriptor rows; the ids come
        back in the rig's numbering (features >= N_left are the right camera's).  cap: the capacity of the handle the key frame was made from."""
        return self.compute_bow(matcher, voc, levelsup, download, cap, "orbx_keyframe_compute_bow_fisheye")

    def bow_from_frame(self, matcher: "ORBmatcher", frame: "DeviceFrame"):
        """The mBowVec / mFeatVec part of KeyFrame::KeyFrame(Frame&) (orbx_keyframe_bow_from_frame): a device-to-device copy of the BoW state of the
        DeviceFrame this key frame was made from (after its compute_bow, before its next load); asynchronous."""
        check(self._L.orbx_keyframe_bow_from_frame(matcher._h, self._h, frame._h), "orbx_keyframe_bow_from_frame")
        return self

    def bow_from_frame_fisheye(self, matcher: "ORBmatcher", frame: "DeviceFrame"):
        """bow_from_frame for a fisheye-stereo key frame and the fisheye handle it was made from (orbx_keyframe_bow_from_frame_fisheye; after the
        handle's compute_bow_fisheye, before its next load); asynchronous."""
        check(self._L.orbx_keyframe_bow_from_frame_fisheye(matcher._h, self._h, frame._h), "orbx_keyframe_bow_from_frame_fisheye")
        return self

    def bow_vector(self, matcher: "ORBmatcher", cap: int | None = None):
        """KeyFrame::mBowVec of a key frame that has BoW (orbx_keyframe_bow_vector): (word_id ascending, value normalised).  cap: the size of the
        buffers while N is on the device only (the capacity of the frame handle the key frame was made from); None = count first."""
        size = max(self.count() if cap is None else int(cap), 1)
        w, v, n = np.zeros(size, np.int32), np.zeros(size, np.float64), C.c_int(0)
        check(self._L.orbx_keyframe_bow_vector(matcher._h, self._h, ptr(w), ptr(v), C.byref(n)), "orbx_keyframe_bow_vector")
        return w[:n.value], v[:n.value]

    def close(self):
        if getattr(self, "_h", None):
            self._L.orbx_keyframe_destroy(self._h)
            self._h = None

    __del__ = close


class DeviceKeyFrameDatabase:
    """The BowVectors of the key frames of a KeyFrameDatabase, resident on the device (orbx_keyframe_database, include/orbx.h): `n_slots` rows of at
    most `words_cap` words, addressed by slot numbers the caller assigns (one int in KeyFrame).  It belongs to no matcher: every ORBmatcher of its
    device may add to it and query it.  add() copies the key frame's BowVector into a slot without waiting; query_frame() / query_keyframe() are the
    first halves of DetectRelocalizationCandidates / DetectNBestCandidates: common words and L1 scores of every slot and the candidates above
    minCommonWords, in one call.  The covisibility accumulation behind them stays on the host.  The caller does not write while a query of another
    thread is running (KeyFrameDatabase::mMutex).  close() (or garbage collection) frees it; no call that was handed it may be running then."""

    def __init__(self, n_slots: int, words_cap: int, device: int = 0):
        self._L = _lib.lib()
        h = C.c_void_p()
        check(self._L.orbx_keyframe_database_create(int(device), int(n_slots), int(words_cap), C.byref(h)), "orbx_keyframe_database_create")
        self._h = h
        self.n_slots, self.words_cap = int(n_slots), int(words_cap)

    def add(self, matcher: "ORBmatcher", slot: int, kf: DeviceKeyFrame):
        """KeyFrameDatabase::add: the key frame's BowVector into `slot` (orbx_keyframe_database_add); returns without waiting."""
        check(self._L.orbx_keyframe_database_add(matcher._h, self._h, int(slot), kf._h), "orbx_keyframe_database_add")
        return self

    def erase(self, matcher: "ORBmatcher", slot: int):
        check(self._L.orbx_keyframe_database_erase(matcher._h, self._h, int(slot)), "orbx_keyframe_database_erase")
        return self

    def clear(self, matcher: "ORBmatcher"):
        check(self._L.orbx_keyframe_database_clear(matcher._h, self._h), "orbx_keyframe_database_clear")
        return self

    def _query(self, fn, matcher, src, exclude, min_ratio, cand_cap, full):
        ex = _i32([] if exclude is None else exclude)
        cap = self.n_slots if cand_cap is None else int(cand_cap)
        common = np.zeros(self.n_slots, np.int32) if full else None
        score = np.zeros(self.n_slots, np.float64) if full else None
        cs, cc, csc = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.float64)
        n_cand, max_common = C.c_int(0), C.c_int(0)
        check(getattr(self._L, fn)(matcher._h, self._h, src._h, ptr(ex) if len(ex) else None, len(ex), float(min_ratio), ptr(common), ptr(score), ptr(cs),
                                   ptr(cc), ptr(csc), cap, C.byref(n_cand), C.byref(max_common)), fn)
        k = min(n_cand.value, cap)
        return dict(n_cand=n_cand.value, max_common=max_common.value, cand_slot=cs[:k], cand_common=cc[:k], cand_score=csc[:k], n_common=common,
                    score=score)

    def query_frame(self, matcher: "ORBmatcher", frame: DeviceFrame, exclude=None, min_ratio: float = 0.8, cand_cap: int | None = None, full: bool = True):
        """KeyFrameDatabase::DetectRelocalizationCandidates' first half for a DeviceFrame after compute_bow (orbx_keyframe_database_query_frame).
        Returns dict(n_cand, max_common, cand_slot, cand_common, cand_score, n_common [n_slots] or None, score [n_slots] or None): the candidates are
        the slots with more than int(float32(max_common) * min_ratio) common words, ascending; n_cand is the true count, the lists hold at most
        cand_cap (None: n_slots) entries.  exclude: slots left out of the count (spConnectedKF)."""
        return self._query("orbx_keyframe_database_query_frame", matcher, frame, exclude, min_ratio, cand_cap, full)

    def query_keyframe(self, matcher: "ORBmatcher", kf: DeviceKeyFrame, exclude=None, min_ratio: float = 0.8, cand_cap: int | None = None, full: bool = True):
        """DetectNBestCandidates' first half for a key frame with BoW, in the database or not (orbx_keyframe_database_query_keyframe)."""
        return self._query("orbx_keyframe_database_query_keyframe", matcher, kf, exclude, min_ratio, cand_cap, full)

    def close(self):
        if getattr(self, "_h", None):
            self._L.orbx_keyframe_database_destroy(self._h)
            self._h = None

    __del__ = close


class DeviceMap:
    """A device-resident table of map points (orbx_map, include/orbx.h): `capacity` slots of pos, normal, min_dist, max_dist and the 32-byte
    descriptor, addressed by ids in [0, capacity) that the caller assigns.  It belongs to no matcher: every ORBmatcher of its device may update and
    read it, and the ...Map forms of the one-call searches take (map, ids) where the flat forms take the five arrays.  What keeps it current:
    ORBmatcher.RefreshMapPointsToMap writes the descriptor, the normal and both distance bounds of the points a LocalMapping step changed
    (ComputeDistinctiveDescriptors + UpdateNormalAndDepth, computed on the device; DistinctiveDescriptorsKeyFramesToMap /
    UpdateNormalAndDepthKeyFramesToMap are its halves); update() is left for SetWorldPos / a bundle adjustment's write-back and for a slot's first,
    whole write; erase() at SetBadFlag.  The caller does not run
    update / erase concurrently with a call that reads the table (the reference's Map::mMutexMapUpdate).  close() (or garbage collection) frees it;
    no call that was handed the table may be running then."""

    def __init__(self, capacity: int, device: int = 0):
        self._L = _lib.lib()
        h = C.c_void_p()
        check(self._L.orbx_map_create(int(device), int(capacity), C.byref(h)), "orbx_map_create")
        self._h = h
        self.capacity = int(capacity)

    def update(self, matcher: "ORBmatcher", ids, pos=None, normal=None, min_dist=None, max_dist=None, desc=None):
        """Row j of the given arrays -> slot ids[j]; None keeps that field (a slot's first update gives all five).  Returns without waiting."""
        i = _i32(ids)
        P = None if pos is None else _f32(np.asarray(pos).reshape(-1, 3))
        Nn = None if normal is None else _f32(np.asarray(normal).reshape(-1, 3))
        mn, mx, d = _f32(min_dist), _f32(max_dist), _u8(desc)
        for a, w in ((P, 3), (Nn, 3), (mn, 1), (mx, 1), (d, 32)):
            assert a is None or a.size == len(i) * w, "one row per id"
        check(self._L.orbx_map_update(matcher._h, self._h, len(i), ptr(i), ptr(P), ptr(Nn), ptr(mn), ptr(mx), ptr(d)), "orbx_map_update")
        return self

    def erase(self, ids):
        i = _i32(ids)
        check(self._L.orbx_map_erase(self._h, len(i), ptr(i)), "orbx_map_erase")
        return self

    def read(self, matcher: "ORBmatcher", ids) -> dict:
        """dict(pos [n, 3], normal [n, 3], min_dist, max_dist, desc [n, 32]) of the slots ids names; one synchronisation."""
        i = _i32(ids)
        n = len(i)
        out = dict(pos=np.zeros((n, 3), np.float32), normal=np.zeros((n, 3), np.float32), min_dist=np.zeros(n, np.float32),
                   max_dist=np.zeros(n, np.float32), desc=np.zeros((n, 32), np.uint8))
        check(self._L.orbx_map_read(matcher._h, self._h, n, ptr(i), ptr(out["pos"]), ptr(out["normal"]), ptr(out["min_dist"]), ptr(out["max_dist"]),
                                    ptr(out["desc"])), "orbx_map_read")
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._L.orbx_map_destroy(self._h)
            self._h = None

    __del__ = close


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, np.int32)


def _u8(a):
    return None if a is None else np.ascontiguousarray(a, np.uint8)


class ORBVocabulary:
    """DBoW2 vocabulary tree on the device (flattened: child CSR, node descriptors, leaf word ids)."""

    def __init__(self, L: int, child_ptr, child_idx, node_desc, word_id, device: int = 0):
        self._L_ = _lib.lib()
        self.L = L
        cp, ci = _i32(child_ptr), _i32(child_idx)
        nd, wi = _u8(node_desc), _i32(word_id)
        self._h = C.c_void_p()
        check(self._L_.orbx_vocabulary_create(device, L, len(wi), ptr(cp), ptr(ci), ptr(nd), ptr(wi), C.byref(self._h)),
              "orbx_vocabulary_create")

    def __del__(self):
        if getattr(self, "_h", None):
            self._L_.orbx_vocabulary_destroy(self._h)
            self._h = None

    def set_word_weights(self, weights):
        """m_words[id]->weight for every word id (orbx_vocabulary_set_word_weights): words with weight <= 0 are stop words for
        DeviceFrame.compute_bow's FeatureVector."""
        w = np.ascontiguousarray(weights, np.float64)
        check(self._L_.orbx_vocabulary_set_word_weights(self._h, ptr(w), len(w)), "orbx_vocabulary_set_word_weights")
        return self


class ORBmatcher:
    TH_LOW = _lib.TH_LOW
    TH_HIGH = _lib.TH_HIGH
    HISTO_LENGTH = _lib.HISTO_LENGTH

    def __init__(self, nnratio: float = 0.6, checkOri: bool = True, device: int = 0):
        self._L = _lib.lib()
        self._h = C.c_void_p()
        check(self._L.orbx_matcher_create(device, C.byref(self._h)), "orbx_matcher_create")
        self.mfNNratio = nnratio
        self.mbCheckOrientation = checkOri
        self._frames = {}   # the live DeviceFrame handles of this matcher

    def __del__(self):
        if getattr(self, "_h", None):
            # A DeviceFrame keeps its owner alive, so it normally goes first.  The collector of reference cycles (a traceback that holds both as
            # locals) finalizes in any order: the handles that are left are destroyed here, ahead of the context their destruction synchronises.
            frames = getattr(self, "_frames", {})
            for h in list(frames.values()):
                self._L.orbx_frame_destroy(h)
            frames.clear()
            self._L.orbx_matcher_destroy(self._h)
            self._h = None

    def last_transfers(self) -> dict:
        """Transfers of the last call: orbx_matcher_debug_transfers (runs up / down, their bytes, how many went through a DMA engine, k_xfer launches)."""
        out = np.zeros(6, np.int64)
        n = self._L.orbx_matcher_debug_transfers(self._h, ptr(out), 6)
        if n < 0:
            raise RuntimeError(f"orbx_matcher_debug_transfers: {n}")
        return {"uploads": int(out[0]), "downloads": int(out[1]), "upload_bytes": int(out[2]), "download_bytes": int(out[3]),
                "dma_submissions": int(out[4]), "xfer_launches": int(out[5])}

    def last_replay_stats(self) -> dict:
        """k_replay_init_lists of the last SearchForInitialization: orbx_matcher_debug_replay_stats."""
        out = np.zeros(3, np.int32)
        if self._L.orbx_matcher_debug_replay_stats(self._h, ptr(out)) < 0:
            raise RuntimeError("orbx_matcher_debug_replay_stats")
        return {"rounds": int(out[0]), "rescans": int(out[1]), "queries": int(out[2])}

    # ---- DescriptorDistance over candidate lists (ORBmatcher.cc:2058-2074) ----
    def hamming_csr(self, q_desc, t_desc, row_ptr, cand):
        q, t, rp, cd = _u8(q_desc), _u8(t_desc), _i32(row_ptr), _i32(cand)
        out = np.zeros(len(cd), np.uint16)
        check(self._L.orbx_hamming_csr(self._h, ptr(q), len(q), ptr(t), len(t), ptr(rp), ptr(cd), ptr(out)),
              "orbx_hamming_csr")
        return out

    def hamming_best2_csr(self, q_desc, t_desc, row_ptr, cand):
        q, t, rp, cd = _u8(q_desc), _u8(t_desc), _i32(row_ptr), _i32(cand)
        o = [np.zeros(len(q), np.int32) for _ in range(4)]
        check(self._L.orbx_hamming_best2_csr(self._h, ptr(q), len(q), ptr(t), len(t), ptr(rp), ptr(cd),
                                             *[ptr(a) for a in o]), "orbx_hamming_best2_csr")
        return tuple(o)

    def knn2(self, q_desc, t_desc):
        """cv::BFMatcher(NORM_HAMMING).knnMatch(q, t, k=2) (Frame.cc:1144)."""
        q, t = _u8(q_desc), _u8(t_desc)
        idx = np.zeros((len(q), 2), np.int32)
        dist = np.zeros((len(q), 2), np.int32)
        check(self._L.orbx_knn2(self._h, ptr(q), len(q), ptr(t), len(t), ptr(idx), ptr(dist)), "orbx_knn2")
        return idx, dist

    def compute_stereo_fisheye_matches(self, kl, dl, mono_left, kr, dr, mono_right, level_sigma2, triangulate):
        """Frame::ComputeStereoFishEyeMatches (Frame.cc:1126-1166): kNN-2 of the lapping-area tails on the device (:1144), Lowe's ratio
        (:1151) and the bookkeeping (:1157-1162) on the host.  triangulate(i_left, i_right, sigma1, sigma2) -> (depth, (x, y, z)) is the
        caller's KannalaBrandt8::TriangulateMatches.  Returns (nMatches, descMatches, l2r, r2l, depth, u_right, p3d)."""
        kl, kr = np.ascontiguousarray(kl, KP_DTYPE), np.ascontiguousarray(kr, KP_DTYPE)
        dl, dr, s2 = _u8(dl), _u8(dr), _f32(level_sigma2)
        n_left, n_right = len(kl), len(kr)
        l2r, r2l = np.full(n_left, -1, np.int32), np.full(n_right, -1, np.int32)
        depth, ur, p3d = np.full(n_left, -1.0, np.float32), np.full(n_left, -1.0, np.float32), np.zeros((n_left, 3), np.float32)
        n_matches = n_desc = 0
        if n_left - mono_left > 0:
            idx, dist = self.knn2(dl[mono_left:], dr[mono_right:])
            for q in range(n_left - mono_left):
                if idx[q, 1] < 0 or not (float(np.float32(dist[q, 0])) < float(np.float32(dist[q, 1])) * 0.7):
                    continue
                n_desc += 1
                il, ir = q + mono_left, int(idx[q, 0]) + mono_right
                d, p = triangulate(il, ir, float(s2[kl["octave"][il]]), float(s2[kr["octave"][ir]]))
                d = np.float32(d)
                if d > np.float32(0.0001):
                    l2r[il], r2l[ir], depth[il], p3d[il] = ir, il, d, np.asarray(p, np.float32)
                    n_matches += 1
        return n_matches, n_desc, l2r, r2l, depth, ur, p3d

    def ComputeStereoFishEyeMatches(self, kl, dl, mono_left, kr, dr, mono_right, level_sigma2, rig):
        """Frame::ComputeStereoFishEyeMatches (Frame.cc:1126-1166) whole on the device: kNN-2 of the lapping-area tails, Lowe's ratio and
        KannalaBrandt8::TriangulateMatches (KannalaBrandt8.cpp:305-368) of the rig's two cameras.  rig: Kb8Rig, or a dataclass / dict with cam_left,
        cam_right (mvParameters), R_lr (mRlr) and t_lr (mtlr).  Returns (nMatches, descMatches, l2r, r2l, depth, u_right (all -1), p3d[n_left, 3])."""
        kl, kr = np.ascontiguousarray(kl, KP_DTYPE), np.ascontiguousarray(kr, KP_DTYPE)
        dl, dr, s2 = _u8(dl), _u8(dr), _f32(level_sigma2)
        n_left, n_right = len(kl), len(kr)
        c = rig if isinstance(rig, _lib.Kb8Rig) else _lib.Kb8Rig.make(rig)
        l2r, r2l = np.full(n_left, -1, np.int32), np.full(n_right, -1, np.int32)
        depth, ur, p3d = np.full(n_left, -1.0, np.float32), np.full(n_left, -1.0, np.float32), np.zeros((n_left, 3), np.float32)
        nd = C.c_int(0)
        n = check(self._L.orbx_compute_stereo_fisheye_matches(self._h, C.byref(c), ptr(kl), ptr(dl), n_left, int(mono_left), ptr(kr), ptr(dr), n_right,
                                                              int(mono_right), ptr(s2), len(s2), ptr(l2r), ptr(r2l), ptr(depth), ptr(p3d),
                                                              C.cast(C.byref(nd), C.c_void_p)), "orbx_compute_stereo_fisheye_matches")
        return n, nd.value, l2r, r2l, depth, ur, p3d

    def stereo_rowband(self, kl, dl, kr, dr, scale_factors, n_rows, min_d, max_d):
        kl = np.ascontiguousarray(kl, KP_DTYPE)
        kr = np.ascontiguousarray(kr, KP_DTYPE)
        dl, dr, sf = _u8(dl), _u8(dr), _f32(scale_factors)
        bi = np.zeros(len(kl), np.int32)
        bd = np.zeros(len(kl), np.int32)
        check(self._L.orbx_stereo_rowband(self._h, ptr(kl), ptr(dl), len(kl), ptr(kr), ptr(dr), len(kr), ptr(sf),
                                          len(sf), n_rows, min_d, max_d, ptr(bi), ptr(bd)), "orbx_stereo_rowband")
        return bi, bd

    def ComputeStereoMatches(self, kl, dl, kr, dr, scale_factors, inv_scale_factors, pyr_left, pyr_right, bf, b):
        """Frame::ComputeStereoMatches (Frame.cc:811-981). pyr_*: lists of level ROI arrays (mvImagePyramid)."""
        kl = np.ascontiguousarray(kl, KP_DTYPE)
        kr = np.ascontiguousarray(kr, KP_DTYPE)
        dl, dr, sf, isf = _u8(dl), _u8(dr), _f32(scale_factors), _f32(inv_scale_factors)
        nl = len(pyr_left)
        pl = (C.c_void_p * nl)(*[p.ctypes.data for p in pyr_left])
        pr = (C.c_void_p * nl)(*[p.ctypes.data for p in pyr_right])
        pw = np.array([p.shape[1] for p in pyr_left], np.int32)
        ph = np.array([p.shape[0] for p in pyr_left], np.int32)
        ps = np.array([p.strides[0] for p in pyr_left], np.uint64)
        for a, b_ in zip(pyr_left, pyr_right):
            assert a.strides == b_.strides and a.strides[1] == 1
        ur = np.zeros(len(kl), np.float32)
        depth = np.zeros(len(kl), np.float32)
        n = check(self._L.orbx_compute_stereo_matches(self._h, ptr(kl), ptr(dl), len(kl), ptr(kr), ptr(dr), len(kr),
                                                      ptr(sf), ptr(isf), nl, C.cast(pl, C.c_void_p),
                                                      C.cast(pr, C.c_void_p), ptr(pw), ptr(ph), ptr(ps), bf, b,
                                                      ptr(ur), ptr(depth)), "orbx_compute_stereo_matches")
        return n, ur, depth

    # ---- SearchByProjection(Frame&, vector<MapPoint*>&, th, ...) (ORBmatcher.cc:43-213) ----
    def SearchByProjection(self, F: FrameView, mp: dict, th: float = 3.0, frame_occupied=None):
        """mp: proj_x, proj_y, proj_xr, level, view_cos, desc, in_view, has_obs.  F: FrameView or DeviceFrame.  Returns (nmatches, frame_match)."""
        n_mp = len(mp["proj_x"])
        a = dict(px=_f32(mp["proj_x"]), py=_f32(mp["proj_y"]), pxr=_f32(mp.get("proj_xr")), lv=_i32(mp["level"]),
                 vc=_f32(mp["view_cos"]), d=_u8(mp["desc"]), iv=_u8(mp.get("in_view")), ho=_u8(mp.get("has_obs")))
        occ = _u8(frame_occupied)
        args = (ptr(occ), n_mp, ptr(a["px"]), ptr(a["py"]), ptr(a["pxr"]), ptr(a["lv"]), ptr(a["vc"]), ptr(a["d"]), ptr(a["iv"]), ptr(a["ho"]),
                th, self.mfNNratio)
        if isinstance(F, DeviceFrame):
            fm = np.full(self._frame_rows(F, occ), -1, np.int32)
            n = check(self._L.orbx_frame_search_by_projection_mappoints(self._h, F._h, *args, ptr(fm)), "orbx_frame_search_by_projection_mappoints")
            return n, fm[:F.count()]
        fd = F.c_struct()
        fm = np.full(fd.n, -1, np.int32)
        n = check(self._L.orbx_search_by_projection_mappoints(self._h, C.byref(fd), *args, ptr(fm)), "orbx_search_by_projection_mappoints")
        return n, fm

    @staticmethod
    def _frame_rows(F: "DeviceFrame", occ) -> int:
        """Rows of a result array for a handle: N when it is known (or must be: an occupancy mask holds N entries), else the capacity."""
        return len(occ) if occ is not None else F.cap

    # ---- SearchByProjection(Frame& Cur, const Frame& Last, th, bMono) (ORBmatcher.cc:1676-1887) ----
    def SearchByProjectionFrame(self, Cur: FrameView, q: dict, th: float, level_mode: int = 0, cur_occupied=None, raw=False):
        """q: u, v, ur, octave, angle, desc, has_obs (last-frame map points already projected into Cur).
        raw=True keeps the C ABI's -2 for "assigned, then cleared by the rotation check" (the slot becomes NULL in the reference)."""
        nq = len(q["u"])
        a = dict(u=_f32(q["u"]), v=_f32(q["v"]), ur=_f32(q.get("ur")), o=_i32(q["octave"]), ang=_f32(q["angle"]),
                 d=_u8(q["desc"]), ho=_u8(q.get("has_obs")))
        occ = _u8(cur_occupied)
        args = (ptr(occ), nq, ptr(a["u"]), ptr(a["v"]), ptr(a["ur"]), ptr(a["o"]), ptr(a["ang"]), ptr(a["d"]), ptr(a["ho"]), th, level_mode,
                int(self.mbCheckOrientation))
        if isinstance(Cur, DeviceFrame):
            cm = np.full(self._frame_rows(Cur, occ), -1, np.int32)
            n = check(self._L.orbx_frame_search_by_projection_frame(self._h, Cur._h, *args, ptr(cm)), "orbx_frame_search_by_projection_frame")
            cm = cm[:Cur.count()]
        else:
            fd = Cur.c_struct()
            cm = np.full(fd.n, -1, np.int32)
            n = check(self._L.orbx_search_by_projection_frame(self._h, C.byref(fd), *args, ptr(cm)), "orbx_search_by_projection_frame")
        return n, (cm if raw else np.maximum(cm, -1))

    # ---- Tracking::SearchLocalPoints (Tracking.cc:3339-3413): isInFrustum + SearchByProjection(F, MPs, th, bFarPoints, thFarPoints) ----
    def SearchLocalPoints(self, F, cam, pose, log_scale_factor, cos_limit, pos, normal, min_dist, max_dist, desc, eligible=None, has_obs=None,
                          th: float = 1.0, far_points: bool = False, th_far_points: float = 0.0, frame_occupied=None):
        """One call, one synchronisation (orbx_frame_search_local_points).  F: DeviceFrame (or a FrameView, loaded into a handle for the call).
        cam = orbx_camera fields (fx, fy, cx, cy, k1, k2, p1, p2, k3, bf); pose = (Rcw, tcw, Ow).  eligible[j] = !isBad() && mnLastFrameSeen != F.mnId,
        has_obs[j] = Observations() > 0.  Returns (nmatches, frame_match[N], in_view[n_mp])."""
        from ._lib import Camera, FramePose
        if not isinstance(F, DeviceFrame):
            F = DeviceFrame(self, max(1, len(F.keypoints_un))).load(F)
        P, Nn = _f32(np.asarray(pos).reshape(-1, 3)), _f32(np.asarray(normal).reshape(-1, 3))
        mn, mx, d, el, ho, occ = _f32(min_dist), _f32(max_dist), _u8(desc), _u8(eligible), _u8(has_obs), _u8(frame_occupied)
        n_mp = len(P)
        iv = np.zeros(n_mp, np.uint8)
        fm = np.full(self._frame_rows(F, occ), -1, np.int32)
        c, p = Camera(*[float(x) for x in cam]), FramePose.make(*pose)
        n = check(self._L.orbx_frame_search_local_points(self._h, F._h, ptr(occ), C.byref(c), C.byref(p), float(log_scale_factor), float(cos_limit),
                                                         n_mp, ptr(P), ptr(Nn), ptr(mn), ptr(mx), ptr(d), ptr(el), ptr(ho), float(th), self.mfNNratio,
                                                         int(bool(far_points)), float(th_far_points), ptr(iv), ptr(fm)),
                  "orbx_frame_search_local_points")
        return n, fm[:F.count()], iv

    # ---- candidate generation: Frame::UndistortKeyPoints / ComputeImageBounds / isInFrustum ----
    def UndistortKeyPoints(self, cam, kps):
        from ._lib import Camera
        k = np.ascontiguousarray(kps, KP_DTYPE)
        out = np.zeros(len(k), KP_DTYPE)
        c = Camera(*[float(x) for x in cam])
        check(self._L.orbx_undistort_keypoints(self._h, C.byref(c), ptr(k), len(k), ptr(out)), "orbx_undistort_keypoints")
        return out

    def ComputeImageBounds(self, cam, width, height):
        from ._lib import Camera
        b = np.zeros(4, np.float32)
        c = Camera(*[float(x) for x in cam])
        check(self._L.orbx_image_bounds(C.byref(c), int(width), int(height), ptr(b)), "orbx_image_bounds")
        return b

    def isInFrustum(self, cam, pose, bounds, log_scale_factor, nlevels, cos_limit, pos, normal, min_dist, max_dist):
        """Frame::isInFrustum for n map points (Nleft == -1).  pose = (Rcw, tcw, Ow).  Returns dict like the oracle's."""
        from ._lib import Camera, FramePose
        P, Nn = _f32(np.asarray(pos).reshape(-1, 3)), _f32(np.asarray(normal).reshape(-1, 3))
        mn, mx, b = _f32(min_dist), _f32(max_dist), _f32(bounds)
        n = len(P)
        # (np.empty: the call writes every entry of every array)
        out = dict(in_view=np.empty(n, np.uint8), proj_x=np.empty(n, np.float32), proj_y=np.empty(n, np.float32), proj_xr=np.empty(n, np.float32),
                   depth=np.empty(n, np.float32), level=np.empty(n, np.int32), view_cos=np.empty(n, np.float32))
        c, p = Camera(*[float(x) for x in cam]), FramePose.make(*pose)
        check(self._L.orbx_is_in_frustum(self._h, C.byref(c), C.byref(p), ptr(b), float(log_scale_factor), int(nlevels), float(cos_limit), n, ptr(P),
                                         ptr(Nn), ptr(mn), ptr(mx), *[ptr(out[k]) for k in ("in_view", "proj_x", "proj_y", "proj_xr", "depth", "level", "view_cos")]),
              "orbx_is_in_frustum")
        return out

    def isInFrustumChecks(self, views, bounds, log_scale_factor, nlevels, cos_limit, pos, normal, min_dist, max_dist):
        """Frame::isInFrustumChecks (Frame.cc:1168) for n map points and the 1 or 2 cameras of a fisheye rig.  views = [(R, t, twc, params8), ...] as the
        reference's lines 1172-1186 compute them.  Returns dict of [n_views][n] arrays: in_view, proj_x, proj_y, depth, level, view_cos."""
        P, Nn = _f32(np.asarray(pos).reshape(-1, 3)), _f32(np.asarray(normal).reshape(-1, 3))
        mn, mx, b = _f32(min_dist), _f32(max_dist), _f32(bounds)
        n, nv = len(P), len(views)
        V = np.ascontiguousarray(np.concatenate([np.concatenate([np.asarray(x, np.float32).ravel() for x in v]) for v in views]), np.float32)
        assert V.size == 23 * nv
        out = dict(in_view=np.empty((nv, n), np.uint8), proj_x=np.empty((nv, n), np.float32), proj_y=np.empty((nv, n), np.float32),
                   depth=np.empty((nv, n), np.float32), level=np.empty((nv, n), np.int32), view_cos=np.empty((nv, n), np.float32))
        check(self._L.orbx_is_in_frustum_checks(self._h, ptr(V), nv, ptr(b), float(log_scale_factor), int(nlevels), float(cos_limit), n, ptr(P), ptr(Nn),
                                                ptr(mn), ptr(mx), *[ptr(out[k]) for k in ("in_view", "proj_x", "proj_y", "depth", "level", "view_cos")]),
              "orbx_is_in_frustum_checks")
        return out

    # ---- fisheye-stereo twins (F.Nleft != -1): features [0, n_left) left camera, [n_left, N) right camera ----
    def SearchByProjectionFisheye(self, left: FrameView, kps_right, l2r, r2l, mp: dict, th: float = 3.0, frame_occupied=None):
        """ORBmatcher.cc:43-213 whole.  left.descriptors holds ALL n_left + n_right rows; mp: in_view, proj_x, proj_y, level,
        view_cos, in_view_r, proj_xr, proj_yr, level_r, view_cos_r, desc, has_obs.  left may be a fisheye DeviceFrame (kps_right, l2r and
        r2l are then the handle's: pass None)."""
        if isinstance(left, DeviceFrame):
            a = [_u8(mp["in_view"]), _f32(mp["proj_x"]), _f32(mp["proj_y"]), _i32(mp["level"]), _f32(mp["view_cos"]), _u8(mp["in_view_r"]),
                 _f32(mp["proj_xr"]), _f32(mp["proj_yr"]), _i32(mp["level_r"]), _f32(mp["view_cos_r"]), _u8(mp["desc"]), _u8(mp.get("has_obs"))]
            occ = _u8(frame_occupied)
            fm = np.full(self._frame_rows(left, occ), -1, np.int32)
            n = check(self._L.orbx_frame_search_by_projection_mappoints_fisheye(self._h, left._h, ptr(occ), len(a[0]), *[ptr(x) for x in a], th,
                                                                                self.mfNNratio, ptr(fm)),
                      "orbx_frame_search_by_projection_mappoints_fisheye")
            return n, fm[:left.count()]
        kr = np.ascontiguousarray(kps_right, KP_DTYPE)
        left.keypoints_un = np.ascontiguousarray(left.keypoints_un, KP_DTYPE)
        fd = left.c_struct()
        N = fd.n + len(kr)
        fm = np.full(N, -1, np.int32)
        a = [_u8(mp["in_view"]), _f32(mp["proj_x"]), _f32(mp["proj_y"]), _i32(mp["level"]), _f32(mp["view_cos"]), _u8(mp["in_view_r"]),
             _f32(mp["proj_xr"]), _f32(mp["proj_yr"]), _i32(mp["level_r"]), _f32(mp["view_cos_r"]), _u8(mp["desc"]), _u8(mp.get("has_obs"))]
        l2r, r2l, occ = _i32(l2r), _i32(r2l), _u8(frame_occupied)
        n = check(self._L.orbx_search_by_projection_mappoints_fisheye(self._h, C.byref(fd), ptr(kr), len(kr), ptr(l2r), ptr(r2l), ptr(occ), len(a[0]),
                                                                      *[ptr(x) for x in a], th, self.mfNNratio, ptr(fm)),
                  "orbx_search_by_projection_mappoints_fisheye")
        return n, fm

    def SearchByProjectionFrameFisheye(self, left: FrameView, kps_right, q: dict, th: float, level_mode: int = 0, cur_occupied=None, raw=False):
        """ORBmatcher.cc:1676-1887 with the twin :1794-1863.  q: u, v, xr, yr, octave, angle, desc, has_obs.  left may be a fisheye
        DeviceFrame (kps_right: None)."""
        if isinstance(left, DeviceFrame):
            a = [_f32(q["u"]), _f32(q["v"]), _f32(q["xr"]), _f32(q["yr"]), _i32(q["octave"]), _f32(q["angle"]), _u8(q["desc"]), _u8(q.get("has_obs"))]
            occ = _u8(cur_occupied)
            cm = np.full(self._frame_rows(left, occ), -1, np.int32)
            n = check(self._L.orbx_frame_search_by_projection_frame_fisheye(self._h, left._h, ptr(occ), len(a[0]), *[ptr(x) for x in a], th, level_mode,
                                                                            int(self.mbCheckOrientation), ptr(cm)),
                      "orbx_frame_search_by_projection_frame_fisheye")
            cm = cm[:left.count()]
            return n, (cm if raw else np.maximum(cm, -1))
        kr = np.ascontiguousarray(kps_right, KP_DTYPE)
        fd = left.c_struct()
        cm = np.full(fd.n + len(kr), -1, np.int32)
        a = [_f32(q["u"]), _f32(q["v"]), _f32(q["xr"]), _f32(q["yr"]), _i32(q["octave"]), _f32(q["angle"]), _u8(q["desc"]), _u8(q.get("has_obs"))]
        occ = _u8(cur_occupied)
        n = check(self._L.orbx_search_by_projection_frame_fisheye(self._h, C.byref(fd), ptr(kr), len(kr), ptr(occ), len(a[0]), *[ptr(x) for x in a],
                                                                  th, level_mode, int(self.mbCheckOrientation), ptr(cm)),
                  "orbx_search_by_projection_frame_fisheye")
        return n, (cm if raw else np.maximum(cm, -1))

    def SearchLocalPointsFisheye(self, F: DeviceFrame, views, log_scale_factor, cos_limit, pos, normal, min_dist, max_dist, desc, eligible=None,
                                 has_obs=None, track_depth=None, th: float = 1.0, far_points: bool = False, th_far_points: float = 0.0,
                                 frame_occupied=None):
        """Tracking::SearchLocalPoints on a fisheye-stereo DeviceFrame in one call (orbx_frame_search_local_points_fisheye).  views = [left, right],
        each (R, t, twc, params8) as isInFrustumChecks.  track_depth = the map points' previous mTrackDepth (read for right-only points; None: such
        a point is never far).  Returns (nmatches, frame_match[N], in_view[2, n_mp])."""
        P, Nn = _f32(np.asarray(pos).reshape(-1, 3)), _f32(np.asarray(normal).reshape(-1, 3))
        mn, mx, d, el, ho, td, occ = _f32(min_dist), _f32(max_dist), _u8(desc), _u8(eligible), _u8(has_obs), _f32(track_depth), _u8(frame_occupied)
        n_mp = len(P)
        V = np.ascontiguousarray(np.concatenate([np.concatenate([np.asarray(x, np.float32).ravel() for x in v]) for v in views]), np.float32)
        assert V.size == 46, "views: left and right camera"
        iv = np.zeros((2, n_mp), np.uint8)
        fm = np.full(self._frame_rows(F, occ), -1, np.int32)
        n = check(self._L.orbx_frame_search_local_points_fisheye(self._h, F._h, ptr(occ), ptr(V), float(log_scale_factor), float(cos_limit), n_mp,
                                                                 ptr(P), ptr(Nn), ptr(mn), ptr(mx), ptr(d), ptr(el), ptr(ho), ptr(td), float(th),
                                                                 self.mfNNratio, int(bool(far_points)), float(th_far_points), ptr(iv), ptr(fm)),
                  "orbx_frame_search_local_points_fisheye")
        return n, fm[:F.count()], iv

    def SearchByBoWFrameFisheye(self, kf_desc, kf_angle, kf_valid, kf_fv: "FeatureVector", f_desc, f_angle, n_f_left: int, f_fv: "FeatureVector"):
        """ORBmatcher.cc:283-392 (frame features >= n_f_left are the right camera's; `|| true` on the right ratio test)."""
        kd, ka, kv, fdsc, fa = _u8(kf_desc), _f32(kf_angle), _u8(kf_valid), _u8(f_desc), _f32(f_angle)
        a, b = kf_fv.c_struct(), f_fv.c_struct()
        fm = np.full(len(fdsc), -1, np.int32)
        n = check(self._L.orbx_search_by_bow_frame_fisheye(self._h, ptr(kd), ptr(ka), ptr(kv), len(kd), C.byref(a), ptr(fdsc), ptr(fa), len(fdsc),
                                                           int(n_f_left), C.byref(b), self.mfNNratio, int(self.mbCheckOrientation), ptr(fm)),
                  "orbx_search_by_bow_frame_fisheye")
        return n, fm

    # ---- general window form: M3 = SearchByProjection(Frame&, KeyFrame*, ...) (ORBmatcher.cc:1889-2010) and
    #      M4 = SearchByProjection(KeyFrame*, Sim3f&, ...) (ORBmatcher.cc:427-646) ----
    @staticmethod
    def _window_args(q: dict, max_dist: float, check_orientation: bool, occ):
        a = dict(x=_f32(q["x"]), y=_f32(q["y"]), r=_f32(q["r"]), lo=_i32(q["min_level"]), hi=_i32(q["max_level"]),
                 ang=_f32(q.get("angle")), d=_u8(q["desc"]), ho=_u8(q.get("has_obs")))
        return a, (ptr(occ), len(q["x"]), ptr(a["x"]), ptr(a["y"]), ptr(a["r"]), ptr(a["lo"]), ptr(a["hi"]), ptr(a["ang"]), ptr(a["d"]),
                   ptr(a["ho"]), max_dist, int(check_orientation))

    def SearchByProjectionWindow(self, F: FrameView, q: dict, max_dist: float, check_orientation: bool, occupied=None, raw=False):
        """q: x, y, r, min_level, max_level, angle, desc[, has_obs].  F: FrameView or DeviceFrame.  raw: see SearchByProjectionFrame."""
        occ = _u8(occupied)
        _keep, args = self._window_args(q, max_dist, check_orientation, occ)
        if isinstance(F, DeviceFrame):
            match = np.full(self._frame_rows(F, occ), -1, np.int32)
            n = check(self._L.orbx_frame_search_by_projection_window(self._h, F._h, *args, ptr(match)), "orbx_frame_search_by_projection_window")
            match = match[:F.count()]
        else:
            fd = F.c_struct()
            match = np.full(fd.n, -1, np.int32)
            n = check(self._L.orbx_search_by_projection_window(self._h, C.byref(fd), *args, ptr(match)), "orbx_search_by_projection_window")
        return n, (match if raw else np.maximum(match, -1))

    def SearchByProjectionWindowFisheye(self, F: DeviceFrame, q: dict, max_dist: float, check_orientation: bool, occupied=None, raw=False):
        """Relocalization's window search on a fisheye-stereo handle (orbx_frame_search_by_projection_window_fisheye): only the left camera is
        searched (GetFeaturesInArea's default bRight = false).  occupied: N entries or None.  Returns (nmatches, match[N]); the right camera's
        entries are -1.  raw: see SearchByProjectionFrame."""
        occ = _u8(occupied)
        _keep, args = self._window_args(q, max_dist, check_orientation, occ)
        match = np.full(self._frame_rows(F, occ), -1, np.int32)
        n = check(self._L.orbx_frame_search_by_projection_window_fisheye(self._h, F._h, *args, ptr(match)),
                  "orbx_frame_search_by_projection_window_fisheye")
        match = match[:F.count()]
        return n, (match if raw else np.maximum(match, -1))

    # ---- SearchForInitialization (ORBmatcher.cc:648-763) ----
    def SearchForInitialization(self, kps1_un, desc1, F2: FrameView, vbPrevMatched, windowSize=100):
        """Returns (nmatches, vnMatches12); vbPrevMatched (n1 x 2 float32) is updated in place."""
        k1 = np.ascontiguousarray(kps1_un, KP_DTYPE)
        d1 = _u8(desc1)
        assert vbPrevMatched.dtype == np.float32 and vbPrevMatched.flags.c_contiguous
        fd = F2.c_struct()
        m12 = np.full(len(k1), -1, np.int32)
        n = check(self._L.orbx_search_for_initialization(self._h, ptr(k1), ptr(d1), len(k1), C.byref(fd), ptr(vbPrevMatched),
                                                         int(windowSize), self.mfNNratio, int(self.mbCheckOrientation),
                                                         ptr(m12)), "orbx_search_for_initialization")
        return n, m12

    # ---- SearchByBoW (ORBmatcher.cc:223-425 / 765-905) ----
    def SearchByBoWFrame(self, kf_desc, kf_angle, kf_valid, kf_fv: FeatureVector, f_desc, f_angle, f_fv: FeatureVector):
        kd, ka, kv, fdsc, fa = _u8(kf_desc), _f32(kf_angle), _u8(kf_valid), _u8(f_desc), _f32(f_angle)
        a, b = kf_fv.c_struct(), f_fv.c_struct()
        fm = np.full(len(fdsc), -1, np.int32)
        n = check(self._L.orbx_search_by_bow_frame(self._h, ptr(kd), ptr(ka), ptr(kv), len(kd), C.byref(a), ptr(fdsc), ptr(fa),
                                                   len(fdsc), C.byref(b), self.mfNNratio, int(self.mbCheckOrientation),
                                                   ptr(fm)), "orbx_search_by_bow_frame")
        return n, fm

    def SearchByBoWDevice(self, F: DeviceFrame, kfs):
        """SearchByBoW(KeyFrame*, Frame&) of the resident frame against every key frame of `kfs` in one call (orbx_frame_search_by_bow; the frame
        needs DeviceFrame.compute_bow first).  kfs: sequence of (desc, angle, valid, FeatureVector) -- valid may be None.
        Returns (nmatches[n_kf], match[n_kf, N]): row k = SearchByBoWFrame for key frame k."""
        return self._search_by_bow_device(F, kfs, "orbx_frame_search_by_bow")

    def SearchByBoWDeviceFisheye(self, F: DeviceFrame, kfs):
        """SearchByBoWDevice for a fisheye-stereo handle (orbx_frame_search_by_bow_fisheye; the frame needs DeviceFrame.compute_bow_fisheye first).
        Returns (nmatches[n_kf], match[n_kf, N]): row k = SearchByBoWFrameFisheye for key frame k (right-camera matches at N_left + j)."""
        return self._search_by_bow_device(F, kfs, "orbx_frame_search_by_bow_fisheye")

    def _search_by_bow_device(self, F: DeviceFrame, kfs, fn: str):
        n_kf = len(kfs)
        keep, arr = [], (BowKeyFrame * max(n_kf, 1))()
        for k, (d, a, v, fv) in enumerate(kfs):
            d, a, v = _u8(d).reshape(-1, 32), _f32(a), _u8(v)
            keep.append((d, a, v, fv))
            arr[k] = BowKeyFrame(d.ctypes.data, None if a is None else a.ctypes.data, None if v is None else v.ctypes.data, len(d), fv.c_struct())
        stride = F.cap
        match = np.full((max(n_kf, 1), stride), -1, np.int32)
        nm = np.zeros(max(n_kf, 1), np.int32)
        check(getattr(self._L, fn)(self._h, F._h, n_kf, arr, self.mfNNratio, int(self.mbCheckOrientation), ptr(match), stride, ptr(nm)), fn)
        del keep
        return nm[:n_kf], match[:n_kf, :F.count()]

    def SearchByBoWKeyFrames(self, desc1, angle1, valid1, fv1: FeatureVector, desc2, angle2, valid2, fv2: FeatureVector):
        d1, a1, v1, d2, a2, v2 = _u8(desc1), _f32(angle1), _u8(valid1), _u8(desc2), _f32(angle2), _u8(valid2)
        a, b = fv1.c_struct(), fv2.c_struct()
        m12 = np.full(len(d1), -1, np.int32)
        n = check(self._L.orbx_search_by_bow_keyframes(self._h, ptr(d1), ptr(a1), ptr(v1), len(d1), C.byref(a), ptr(d2),
                                                       ptr(a2), ptr(v2), len(d2), C.byref(b), self.mfNNratio,
                                                       int(self.mbCheckOrientation), ptr(m12)),
                  "orbx_search_by_bow_keyframes")
        return n, m12

    # ---- the BoW-guided matchers with both sides resident (DeviceKeyFrames with BoW) ----
    @staticmethod
    def _kf_handles(kfs):
        vp = C.c_void_p
        return (vp * max(len(kfs), 1))(*[kf._h.value if isinstance(kf._h, vp) else kf._h for kf in kfs])

    @staticmethod
    def _flag_rows(flags, K):
        keep = [None] * K if flags is None else [_u8(v) for v in flags]
        assert len(keep) == K
        return keep, (C.c_void_p * max(K, 1))(*[None if v is None else v.ctypes.data for v in keep])

    def SearchByBoWResident(self, F: DeviceFrame, kfs, valid=None, fn: str = "orbx_frame_search_by_bow_resident"):
        """SearchByBoW(KeyFrame*, Frame&) of the resident frame against DeviceKeyFrames that carry BoW, in one call (orbx_frame_search_by_bow_resident).
        valid: per key frame a uint8[N_k] mask or None (all), or None for all key frames.  Returns (nmatches[K], match[K, N]): row k =
        SearchByBoWFrame for key frame k's host arrays.  Only the masks and one record per key frame are uploaded."""
        K = len(kfs)
        keep, rows = self._flag_rows(valid, K)
        stride = F.cap
        match = np.full((max(K, 1), stride), -1, np.int32)
        nm = np.zeros(max(K, 1), np.int32)
        check(getattr(self._L, fn)(self._h, F._h, K, self._kf_handles(kfs), rows, self.mfNNratio, int(self.mbCheckOrientation), ptr(match), stride,
                                   ptr(nm)), fn)
        del keep
        return nm[:K], match[:K, :F.count()]

    def SearchByBoWResidentFisheye(self, F: DeviceFrame, kfs, valid=None):
        """SearchByBoWResident of a fisheye-stereo handle against fisheye-stereo DeviceKeyFrames that carry BoW
        (orbx_frame_search_by_bow_resident_fisheye): row k = SearchByBoWFrameFisheye for key frame k's host arrays, features in the rig's numbering
        on both sides."""
        return self.SearchByBoWResident(F, kfs, valid, "orbx_frame_search_by_bow_resident_fisheye")

    def SearchByBoWKeyFramesResident(self, kf1: DeviceKeyFrame, kfs2, valid1=None, valid2=None, fn: str = "orbx_keyframe_search_by_bow"):
        """SearchByBoW(pKF1, pKF2) for kf1 against every key frame of kfs2 in one call (orbx_keyframe_search_by_bow).  Returns (nmatches[K],
        match12[K, N1]): row k = SearchByBoWKeyFrames(kf1, kfs2[k]) on host arrays."""
        K = len(kfs2)
        v1 = _u8(valid1)
        keep, rows = self._flag_rows(valid2, K)
        n1 = kf1.count()
        match = np.full((max(K, 1), max(n1, 1)), -1, np.int32)
        nm = np.zeros(max(K, 1), np.int32)
        check(getattr(self._L, fn)(self._h, kf1._h, ptr(v1), K, self._kf_handles(kfs2), rows, self.mfNNratio, int(self.mbCheckOrientation), ptr(match),
                                   max(n1, 1), ptr(nm)), fn)
        del keep
        return nm[:K], match[:K, :n1]

    def SearchByBoWKeyFramesResidentFisheye(self, kf1: DeviceKeyFrame, kfs2, valid1=None, valid2=None):
        """SearchByBoW(pKF1, pKF2) between fisheye-stereo key frames (orbx_keyframe_search_by_bow_fisheye): the right camera's features are neither
        queries nor candidates (ORBmatcher.cc:800-802, :820-822), so rows >= N_left1 are -1 and values are below N_left2."""
        return self.SearchByBoWKeyFramesResident(kf1, kfs2, valid1, valid2, "orbx_keyframe_search_by_bow_fisheye")

    def SearchForTriangulationResidentKB8(self, kf1: DeviceKeyFrame, kf2: DeviceKeyFrame, skip1, skip2, level_sigma2_1, level_sigma2_2, cam1, cam2, R12,
                                          t12, coarse=False):
        """SearchForTriangulationKB8 between two resident fisheye-stereo key frames (orbx_keyframe_search_for_triangulation_fisheye): keypoints,
        descriptors and FeatureVectors are the key frames' own.  Returns (nmatches, matches12[N1]), values in kf2's features [0, N2)."""
        s1, s2, sg1, sg2 = _u8(skip1), _u8(skip2), _f32(level_sigma2_1), _f32(level_sigma2_2)
        flat = lambda x, n: (C.c_float * n)(*[float(v) for v in np.asarray(x, np.float32).ravel()])
        g = KeyFrameKb8Gate(sg1.ctypes.data, sg2.ctypes.data, len(sg1), flat(cam1, 16), flat(cam2, 16), flat(R12, 36), flat(t12, 12), int(coarse))
        n1 = kf1.count()
        m12 = np.full(max(n1, 1), -1, np.int32)
        n = check(self._L.orbx_keyframe_search_for_triangulation_fisheye(self._h, kf1._h, kf2._h, ptr(s1), ptr(s2), int(self.mbCheckOrientation),
                                                                         C.byref(g), ptr(m12)), "orbx_keyframe_search_for_triangulation_fisheye")
        return n, m12[:n1]

    def SearchForTriangulationResident(self, kf1: DeviceKeyFrame, kf2: DeviceKeyFrame, skip1, skip2, level_sigma2_2, F12, epipole, coarse=False,
                                       strict_fp=False):
        """SearchForTriangulationPinhole between two resident key frames (orbx_keyframe_search_for_triangulation): keypoints, mvuRight, descriptors,
        FeatureVectors and scale factors are the key frames' own; level_sigma2_2 = pKF2->mvLevelSigma2.  Returns (nmatches, matches12[N1])."""
        s1, s2, sg = _u8(skip1), _u8(skip2), _f32(level_sigma2_2)
        g = KeyFrameGate((C.c_float * 9)(*[float(x) for x in np.asarray(F12, np.float32).ravel()]), float(epipole[0]), float(epipole[1]), int(coarse),
                         int(strict_fp), len(sg), sg.ctypes.data)
        m12 = np.full(max(kf1.count(), 1), -1, np.int32)
        n = check(self._L.orbx_keyframe_search_for_triangulation(self._h, kf1._h, kf2._h, ptr(s1), ptr(s2), int(self.mbCheckOrientation), C.byref(g),
                                                                 ptr(m12)), "orbx_keyframe_search_for_triangulation")
        return n, m12[:kf1.count()]

    # ---- LocalMapping::CreateNewMapPoints' triangulation on resident key frames (include/orbx.h; PARITY UNPINNED) ----
    @staticmethod
    def _new_points_params(kf1, kf2, level_sigma2_1, level_sigma2_2, ratio_factor, inertial, far_points, th_far_points):
        sg1, sg2 = _f32(level_sigma2_1), _f32(level_sigma2_2)
        return (sg1, sg2), NewPointsParams(float(ratio_factor), int(bool(inertial)), int(bool(far_points)), float(th_far_points), len(sg1), len(sg2),
                                           sg1.ctypes.data, sg2.ctypes.data)

    @staticmethod
    def _new_points_views(views1, views2, rig: bool):
        """Pinhole: a view is (Rcw, tcw, Ow, fx, fy, cx, cy); a rig: (left, right) per key frame, each (R, t, twc, params8) as orbx_fisheye_view.
        A caller that triangulates against the same poses again may pass what NewPointsViews returned: nothing is converted then."""
        if isinstance(views1, NewPointsView) or (isinstance(views1, np.ndarray) and views1.dtype == np.float32 and views1.shape == (46,)):
            return (views1, views2), ((ptr(views1), ptr(views2)) if rig else (C.byref(views1), C.byref(views2)))
        if rig:
            flat = [np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).ravel() for cam in v for x in cam])) for v in (views1, views2)]
            assert all(len(f) == 46 for f in flat), "two orbx_fisheye_view per key frame"
            return flat, (ptr(flat[0]), ptr(flat[1]))
        vs = [NewPointsView((C.c_float * 9)(*[float(x) for x in np.asarray(v[0], np.float32).ravel()]), (C.c_float * 3)(*[float(x) for x in v[1]]),
                            (C.c_float * 3)(*[float(x) for x in v[2]]), float(v[3]), float(v[4]), float(v[5]), float(v[6])) for v in (views1, views2)]
        return vs, (C.byref(vs[0]), C.byref(vs[1]))

    @classmethod
    def NewPointsViews(cls, views1, views2, rig: bool = False):
        """The two key frames' views in the form the four calls below hand to the library, for reuse over several calls."""
        return cls._new_points_views(views1, views2, rig)[0]

    def UnprojectStereo(self, frame: DeviceFrame, view, pos=None):
        """Frame::UnprojectStereo for every feature of a resident frame that holds mvDepth (orbx_frame_unproject_stereo): view = (Rcw, tcw, Ow, fx, fy,
        cx, cy) or a NewPointsView.  pos (optional, [cap, 3] float32): rows of features with depth > 0 are written, the others keep their values.
        Returns (n_with_depth, mvuRight [N], mvDepth [N], pos [N, 3])."""
        v = view if isinstance(view, NewPointsView) else self._new_points_views(view, view, False)[0][0]
        out = np.zeros((frame.cap, 3), np.float32) if pos is None else pos
        assert out.dtype == np.float32 and out.shape == (frame.cap, 3) and out.flags.c_contiguous
        ur, depth = np.zeros(frame.cap, np.float32), np.zeros(frame.cap, np.float32)
        with_depth = C.c_int(0)
        check(self._L.orbx_frame_unproject_stereo(self._h, frame._h, C.byref(v), ptr(ur), ptr(depth), ptr(out), C.byref(with_depth)),
              "orbx_frame_unproject_stereo")
        n = frame.count()   # (known after the call: no further synchronisation)
        return with_depth.value, ur[:n], depth[:n], out[:n]

    def TriangulatePairsKeyFrames(self, kf1: DeviceKeyFrame, kf2: DeviceKeyFrame, view1, view2, level_sigma2_1, level_sigma2_2, ratio_factor, idx1, idx2,
                                  inertial=False, far_points=False, th_far_points=0.0, pos=None, rig: bool = False, stereo=None):
        """The loop body of LocalMapping::CreateNewMapPoints for the pairs (idx1[p], idx2[p]) of two resident key frames
        (orbx_keyframe_triangulate_pairs): unprojection, parallax test, GeometricTools::Triangulate, depth, reprojection, distance and scale-ratio
        tests on the device.  ratio_factor = 1.5f * mfScaleFactor of kf1; idx2[p] = -1: no match.  pos (optional, [n, 3] float32): rows of accepted pairs
        are written, the others keep their values.  Returns (n_accepted, pos [n, 3], status [n] of _lib.NEWPT_*)."""
        i1, i2 = _i32(idx1), _i32(idx2)
        n = len(i1)
        assert len(i2) == n
        keep, par = self._new_points_params(kf1, kf2, level_sigma2_1, level_sigma2_2, ratio_factor, inertial, far_points, th_far_points)
        vkeep, (v1, v2) = self._new_points_views(view1, view2, rig)
        out = np.zeros((n, 3), np.float32) if pos is None else pos
        assert out.dtype == np.float32 and out.shape == (n, 3) and out.flags.c_contiguous
        status = np.zeros(n, np.uint8)
        acc = C.c_int32(0)
        fn = "orbx_keyframe_triangulate_pairs_fisheye" if rig else "orbx_keyframe_triangulate_pairs_stereo" if stereo is not None else "orbx_keyframe_triangulate_pairs"
        extra = () if stereo is None else (C.byref(stereo),)   # (`st` follows `par`)
        check(getattr(self._L, fn)(self._h, kf1._h, kf2._h, v1, v2, C.byref(par), *extra, n, ptr(i1), ptr(i2), ptr(out), ptr(status), C.byref(acc)), fn)
        del keep, vkeep
        return acc.value, out, status

    def TriangulatePairsKeyFramesKB8(self, kf1: DeviceKeyFrame, kf2: DeviceKeyFrame, views1, views2, level_sigma2_1, level_sigma2_2, ratio_factor, idx1,
                                     idx2, inertial=False, far_points=False, th_far_points=0.0, pos=None):
        """The same between two fisheye-stereo key frames (orbx_keyframe_triangulate_pairs_fisheye): views1 / views2 = (left, right) of each key frame,
        each (R, t, twc, params8) -- GetPose() / GetRightPose(), GetCameraCenter() / GetRightCameraCenter(), mpCamera / mpCamera2; an index from
        N_left on is the right camera's."""
        return self.TriangulatePairsKeyFrames(kf1, kf2, views1, views2, level_sigma2_1, level_sigma2_2, ratio_factor, idx1, idx2, inertial, far_points,
                                              th_far_points, pos, rig=True)

    def TriangulatePairsKeyFramesStereo(self, kf1: DeviceKeyFrame, kf2: DeviceKeyFrame, view1, view2, level_sigma2_1, level_sigma2_2, ratio_factor, mb1, mbf1,
                                        mb2, mbf2, idx1, idx2, inertial=False, far_points=False, th_far_points=0.0, pos=None):
        """TriangulatePairsKeyFrames with the member's stereo branches (orbx_keyframe_triangulate_pairs_stereo): mb / mbf = KeyFrame::mb, mbf of each key
        frame.  A pair with mvuRight >= 0 on a key frame that holds mvDepth (create_host_stereo, from_frame of a depth handle) is decided on the
        device -- triangulated, or unprojected from its depth (NEWPT_UNPROJECT_FAILED where mvDepth <= 0)."""
        st = NewPointsStereo(float(mb1), float(mbf1), float(mb2), float(mbf2))
        return self.TriangulatePairsKeyFrames(kf1, kf2, view1, view2, level_sigma2_1, level_sigma2_2, ratio_factor, idx1, idx2, inertial, far_points,
                                              th_far_points, pos, stereo=st)

    def _search_and_triangulate(self, fn, kf1, kf2, skip1, skip2, gate, views, par, pos, stereo=None):
        s1, s2 = _u8(skip1), _u8(skip2)
        n1 = kf1.count()
        m12 = np.full(max(n1, 1), -1, np.int32)
        out = np.zeros((max(n1, 1), 3), np.float32) if pos is None else pos
        assert out.dtype == np.float32 and out.shape == (max(n1, 1), 3) and out.flags.c_contiguous
        status = np.zeros(max(n1, 1), np.uint8)
        acc = C.c_int32(0)
        extra = () if stereo is None else (C.byref(stereo),)   # (`st` follows `par`)
        n = check(getattr(self._L, fn)(self._h, kf1._h, kf2._h, ptr(s1), ptr(s2), int(self.mbCheckOrientation), C.byref(gate), views[0], views[1],
                                       C.byref(par), *extra, ptr(m12), ptr(out), ptr(status), C.byref(acc)), fn)
        return n, m12[:n1], acc.value, out[:n1], status[:n1]

    def SearchAndTriangulateResident(self, kf1: DeviceKeyFrame, kf2: DeviceKeyFrame, skip1, skip2, level_sigma2_1, level_sigma2_2, F12, epipole, view1,
                                     view2, ratio_factor, coarse=False, strict_fp=False, inertial=False, far_points=False, th_far_points=0.0, pos=None,
                                     stereo=None):
        """SearchForTriangulationResident and TriangulatePairsKeyFrames on its match row in one call (orbx_keyframe_search_and_triangulate): one
        launch more than the search, one synchronisation.  Returns (nmatches, matches12 [N1], n_accepted, pos [N1, 3], status [N1])."""
        keep, par = self._new_points_params(kf1, kf2, level_sigma2_1, level_sigma2_2, ratio_factor, inertial, far_points, th_far_points)
        g = KeyFrameGate((C.c_float * 9)(*[float(x) for x in np.asarray(F12, np.float32).ravel()]), float(epipole[0]), float(epipole[1]), int(coarse),
                         int(strict_fp), len(keep[1]), keep[1].ctypes.data)
        vkeep, views = self._new_points_views(view1, view2, False)
        fn = "orbx_keyframe_search_and_triangulate" if stereo is None else "orbx_keyframe_search_and_triangulate_stereo"
        r = self._search_and_triangulate(fn, kf1, kf2, skip1, skip2, g, views, par, pos, stereo)
        del keep, vkeep
        return r

    def SearchAndTriangulateResidentStereo(self, kf1: DeviceKeyFrame, kf2: DeviceKeyFrame, skip1, skip2, level_sigma2_1, level_sigma2_2, F12, epipole, view1,
                                           view2, ratio_factor, mb1, mbf1, mb2, mbf2, coarse=False, strict_fp=False, inertial=False, far_points=False,
                                           th_far_points=0.0, pos=None):
        """SearchAndTriangulateResident with the member's stereo branches (orbx_keyframe_search_and_triangulate_stereo): the row and the return value are
        the plain search's, pos / status those of TriangulatePairsKeyFramesStereo on that row."""
        st = NewPointsStereo(float(mb1), float(mbf1), float(mb2), float(mbf2))
        return self.SearchAndTriangulateResident(kf1, kf2, skip1, skip2, level_sigma2_1, level_sigma2_2, F12, epipole, view1, view2, ratio_factor, coarse,
                                                 strict_fp, inertial, far_points, th_far_points, pos, stereo=st)

    def SearchAndTriangulateResidentKB8(self, kf1: DeviceKeyFrame, kf2: DeviceKeyFrame, skip1, skip2, level_sigma2_1, level_sigma2_2, cam1, cam2, R12, t12,
                                        views1, views2, ratio_factor, coarse=False, inertial=False, far_points=False, th_far_points=0.0, pos=None):
        """SearchForTriangulationResidentKB8 and TriangulatePairsKeyFramesKB8 on its match row in one call
        (orbx_keyframe_search_and_triangulate_fisheye).  Returns (nmatches, matches12 [N1], n_accepted, pos [N1, 3], status [N1])."""
        keep, par = self._new_points_params(kf1, kf2, level_sigma2_1, level_sigma2_2, ratio_factor, inertial, far_points, th_far_points)
        flat = lambda x, n: (C.c_float * n)(*[float(v) for v in np.asarray(x, np.float32).ravel()])
        g = KeyFrameKb8Gate(keep[0].ctypes.data, keep[1].ctypes.data, len(keep[0]), flat(cam1, 16), flat(cam2, 16), flat(R12, 36), flat(t12, 12), int(coarse))
        vkeep, views = self._new_points_views(views1, views2, True)
        r = self._search_and_triangulate("orbx_keyframe_search_and_triangulate_fisheye", kf1, kf2, skip1, skip2, g, views, par, pos)
        del keep, vkeep
        return r

    # ---- SearchForTriangulation (ORBmatcher.cc:907-1146) ----
    def SearchForTriangulation(self, desc1, angle1, skip1, fv1: FeatureVector, desc2, angle2, skip2, fv2: FeatureVector,
                               pair_ok=None):
        """pair_ok(idx1, idx2) -> bool: the geometric gates (epipole distance + epipolarConstrain, or bCoarse)."""
        d1, a1, s1, d2, a2, s2 = _u8(desc1), _f32(angle1), _u8(skip1), _u8(desc2), _f32(angle2), _u8(skip2)
        a, b = fv1.c_struct(), fv2.c_struct()
        m12 = np.full(len(d1), -1, np.int32)
        cb = PAIR_PREDICATE((lambda user, i, j: int(bool(pair_ok(i, j)))) if pair_ok else 0)
        n = check(self._L.orbx_search_for_triangulation(self._h, ptr(d1), ptr(a1), ptr(s1), len(d1), C.byref(a), ptr(d2),
                                                        ptr(a2), ptr(s2), len(d2), C.byref(b), int(self.mbCheckOrientation),
                                                        cb, None, ptr(m12)), "orbx_search_for_triangulation")
        return n, m12

    def SearchForTriangulationPinhole(self, kps1_un, desc1, skip1, fv1: FeatureVector, kps2_un, desc2, skip2, fv2: FeatureVector,
                                      scale_factors2, level_sigma2_2, F12, epipole, u_right1=None, u_right2=None, coarse=False,
                                      strict_fp=False):
        """SearchForTriangulation for pinhole key frames with the epipole-distance test (ORBmatcher.cc:1026-1034) and
        Pinhole::epipolarConstrain (Pinhole.cpp:107-129, on the caller's F12) evaluated on the device: no callback."""
        k1, k2 = np.ascontiguousarray(kps1_un, KP_DTYPE), np.ascontiguousarray(kps2_un, KP_DTYPE)
        d1, s1, d2, s2 = _u8(desc1), _u8(skip1), _u8(desc2), _u8(skip2)
        sf, sg = _f32(scale_factors2), _f32(level_sigma2_2)
        ur1, ur2 = _f32(u_right1), _f32(u_right2)
        g = PinholeGate(k1.ctypes.data, k2.ctypes.data, None if ur1 is None else ur1.ctypes.data, None if ur2 is None else ur2.ctypes.data,
                        sf.ctypes.data, sg.ctypes.data, len(sf), (C.c_float * 9)(*[float(x) for x in np.asarray(F12, np.float32).ravel()]),
                        float(epipole[0]), float(epipole[1]), int(coarse), int(strict_fp))
        a, b = fv1.c_struct(), fv2.c_struct()
        m12 = np.full(len(k1), -1, np.int32)
        n = check(self._L.orbx_search_for_triangulation_pinhole(self._h, ptr(d1), ptr(s1), len(k1), C.byref(a), ptr(d2), ptr(s2), len(k2),
                                                                C.byref(b), int(self.mbCheckOrientation), C.byref(g), ptr(m12)),
                  "orbx_search_for_triangulation_pinhole")
        return n, m12

    def SearchForTriangulationKB8(self, kps1, n_left1, desc1, skip1, fv1: FeatureVector, kps2, n_left2, desc2, skip2, fv2: FeatureVector,
                                  level_sigma2_1, level_sigma2_2, cam1, cam2, R12, t12, coarse=False):
        """SearchForTriangulation between key frames of a fisheye rig: KannalaBrandt8::epipolarConstrain (ORBmatcher.cc:1036-1072) on the device.
        kps: mvKeys | mvKeysRight; cam1 / cam2: [2][8] parameters of (mpCamera, mpCamera2); R12 [4][3][3], t12 [4][3] = ll, lr, rl, rr."""
        from ._lib import Kb8GateStruct
        k1, k2 = np.ascontiguousarray(kps1, KP_DTYPE), np.ascontiguousarray(kps2, KP_DTYPE)
        d1, s1, d2, s2 = _u8(desc1), _u8(skip1), _u8(desc2), _u8(skip2)
        sg1, sg2 = _f32(level_sigma2_1), _f32(level_sigma2_2)
        flat = lambda x, n: (C.c_float * n)(*[float(v) for v in np.asarray(x, np.float32).ravel()])
        g = Kb8GateStruct(k1.ctypes.data, k2.ctypes.data, int(n_left1), int(n_left2), sg1.ctypes.data, sg2.ctypes.data, len(sg1), flat(cam1, 16), flat(cam2, 16),
                          flat(R12, 36), flat(t12, 12), int(coarse))
        a, b = fv1.c_struct(), fv2.c_struct()
        m12 = np.full(len(k1), -1, np.int32)
        n = check(self._L.orbx_search_for_triangulation_kb8(self._h, ptr(d1), ptr(s1), len(k1), C.byref(a), ptr(d2), ptr(s2), len(k2), C.byref(b),
                                                            int(self.mbCheckOrientation), C.byref(g), ptr(m12)), "orbx_search_for_triangulation_kb8")
        return n, m12

    def DebugKb8Epipolar(self, cam1, cam2, R12, t12, xy1, xy2, sigma1, sigma2, sel):
        """Test hook: KannalaBrandt8::epipolarConstrain of n independent pairs on the device (orbx_debug_kb8_epipolar); returns ok uint8[n]."""
        c1, c2, R, t = (np.ascontiguousarray(x, np.float32).ravel() for x in (cam1, cam2, R12, t12))
        assert len(c1) == 16 and len(c2) == 16 and len(R) == 36 and len(t) == 12
        a, b = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2), np.ascontiguousarray(xy2, np.float32).reshape(-1, 2)
        s1, s2, se = _f32(sigma1), _f32(sigma2), _u8(sel)
        ok = np.zeros(len(a), np.uint8)
        check(self._L.orbx_debug_kb8_epipolar(self._h, ptr(c1), ptr(c2), ptr(R), ptr(t), len(a), ptr(a), ptr(b), ptr(s1), ptr(s2), ptr(se), ptr(ok)),
              "orbx_debug_kb8_epipolar")
        return ok

    # ---- DBoW2 transform (Frame::ComputeBoW, Frame.cc:738-745) ----
    def BowTransform(self, voc: "ORBVocabulary", descriptors, levelsup: int = 4):
        """Returns (word_id[n], node_id[n]) of TemplatedVocabulary::transform for every descriptor."""
        d = _u8(descriptors)
        w = np.zeros(len(d), np.int32)
        nd = np.zeros(len(d), np.int32)
        check(self._L.orbx_bow_transform(self._h, voc._h, ptr(d), len(d), levelsup, ptr(w), ptr(nd)), "orbx_bow_transform")
        return w, nd

    # ---- MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:329-403), batched ----
    def DistinctiveDescriptors(self, descriptors, set_ptr):
        d, sp = _u8(descriptors), _i32(set_ptr)
        out = np.zeros(len(sp) - 1, np.int32)
        check(self._L.orbx_distinctive_descriptors(self._h, ptr(d), ptr(sp), len(sp) - 1, ptr(out)), "orbx_distinctive_descriptors")
        return out

    def DistinctiveDescriptorsKeyFrames(self, kfs, set_ptr, obs_kf, obs_idx, want_desc: bool = True):
        """ComputeDistinctiveDescriptors with the observations named where they are (orbx_keyframe_distinctive_descriptors): observation o of set s,
        o in [set_ptr[s], set_ptr[s+1]), is row obs_idx[o] of mDescriptors of the DeviceKeyFrame kfs[obs_kf[o]] (both kinds may be mixed; a rig key
        frame in its own numbering, left then right).  No row is uploaded.  Returns (best_obs[n_sets]: the winner's position inside its set, -1 for
        an empty set; best_desc[n_sets, 32]: the winning rows, zeros for an empty set, or None)."""
        sp, ok, oi = _i32(set_ptr), _i32(obs_kf), _i32(obs_idx)
        n_sets = len(sp) - 1
        assert n_sets >= 0 and len(ok) == len(oi) and (n_sets == 0 or sp[-1] <= len(ok))
        best = np.full(n_sets, -1, np.int32)
        desc = np.zeros((n_sets, 32), np.uint8) if want_desc else None
        check(self._L.orbx_keyframe_distinctive_descriptors(self._h, len(kfs), self._kf_handles(kfs), n_sets, ptr(sp), ptr(ok), ptr(oi), ptr(best),
                                                            ptr(desc)), "orbx_keyframe_distinctive_descriptors")
        return best, desc

    # ---- matching core of Fuse x2 (ORBmatcher.cc:1148-1455) ----
    def FuseSearch(self, KF: FrameView, q: dict, inv_level_sigma2=None, strict_fp: bool = False):
        """q: u, v, ur, r, level, desc.  Returns (best_idx[nq], best_dist[nq])."""
        fd = KF.c_struct()
        nq = len(q["u"])
        a = dict(u=_f32(q["u"]), v=_f32(q["v"]), ur=_f32(q.get("ur")), r=_f32(q["r"]), lv=_i32(q["level"]), d=_u8(q["desc"]))
        isg = _f32(inv_level_sigma2)
        bi = np.zeros(nq, np.int32)
        bd = np.zeros(nq, np.int32)
        check(self._L.orbx_fuse_search(self._h, C.byref(fd), ptr(isg), nq, ptr(a["u"]), ptr(a["v"]), ptr(a["ur"]), ptr(a["r"]),
                                       ptr(a["lv"]), ptr(a["d"]), int(strict_fp), ptr(bi), ptr(bd)), "orbx_fuse_search")
        return bi, bd

    # ---- Fuse on resident key frames: K targets in one call (LocalMapping::SearchInNeighbors) ----
    def FuseSearchKeyFrames(self, kfs, queries, use_chi2: bool = True, strict_fp: bool = False):
        """FuseSearch for K DeviceKeyFrames in one call (orbx_keyframe_fuse_search).  queries[k]: dict(u, v, ur, r, level, desc) of key frame k
        (ur may be None).  use_chi2: the reprojection gate with the key frames' inv_level_sigma2; False = the gate-less form (Fuse with a Sim3,
        SearchBySim3).  Returns [(best_idx, best_dist)] per key frame, each equal to FuseSearch on that key frame's host arrays."""
        K = len(kfs)
        assert len(queries) == K
        keep, qs = [], (FuseQueries * max(K, 1))()
        bi, bd = [], []
        for k, q in enumerate(queries):
            nq = len(q["u"])
            a = [_f32(q["u"]), _f32(q["v"]), _f32(q.get("ur")), _f32(q["r"]), _i32(q["level"]), _u8(q["desc"])]
            keep.append(a)
            qs[k] = FuseQueries(nq, *[None if (x is None or nq == 0) else x.ctypes.data for x in a])
            bi.append(np.zeros(nq, np.int32))
            bd.append(np.zeros(nq, np.int32))
        vp = C.c_void_p
        hs = (vp * max(K, 1))(*[kf._h.value if isinstance(kf._h, vp) else kf._h for kf in kfs])
        pi = (vp * max(K, 1))(*[ptr(x) for x in bi])
        pd = (vp * max(K, 1))(*[ptr(x) for x in bd])
        check(self._L.orbx_keyframe_fuse_search(self._h, K, hs, qs, int(bool(use_chi2)), int(bool(strict_fp)), pi, pd), "orbx_keyframe_fuse_search")
        return list(zip(bi, bd))

    def FuseSearchKeyFramesFisheye(self, kfs, queries, use_chi2: bool = True, strict_fp: bool = False):
        """FuseSearchKeyFrames for K fisheye-stereo DeviceKeyFrames (orbx_keyframe_fuse_search_fisheye).  queries[k] = (left set, right set), each a
        dict(u, v, r, level, desc).  Returns [((best_idx, best_dist) left, (best_idx, best_dist) right)] per key frame; a right-camera index is
        N_left + j."""
        K = len(kfs)
        assert len(queries) == K and all(len(q) == 2 for q in queries)
        keep, qs = [], (FuseQueries * max(2 * K, 1))()
        bi, bd = [], []
        for p, q in enumerate(q for pair in queries for q in pair):
            nq = len(q["u"])
            a = [_f32(q["u"]), _f32(q["v"]), None, _f32(q["r"]), _i32(q["level"]), _u8(q["desc"])]
            keep.append(a)
            qs[p] = FuseQueries(nq, *[None if (x is None or nq == 0) else x.ctypes.data for x in a])
            bi.append(np.zeros(nq, np.int32))
            bd.append(np.zeros(nq, np.int32))
        vp = C.c_void_p
        hs = (vp * max(K, 1))(*[kf._h.value if isinstance(kf._h, vp) else kf._h for kf in kfs])
        pi = (vp * max(2 * K, 1))(*[ptr(x) for x in bi])
        pd = (vp * max(2 * K, 1))(*[ptr(x) for x in bd])
        check(self._L.orbx_keyframe_fuse_search_fisheye(self._h, K, hs, qs, int(bool(use_chi2)), int(bool(strict_fp)), pi, pd),
              "orbx_keyframe_fuse_search_fisheye")
        return [((bi[2 * k], bd[2 * k]), (bi[2 * k + 1], bd[2 * k + 1])) for k in range(K)]

    def FuseMapPointsFisheye(self, kfs, views, map_points: dict, th: float = 3.0, log_scale_factor: float = 0.0, skip=None,
                             strict_fp: bool = False, want_projected: bool = True):
        """Both Fuse calls of LocalMapping::SearchInNeighbors' loop on a rig, for K fisheye-stereo DeviceKeyFrames in one call, projection included
        (orbx_keyframe_fuse_map_points_fisheye).  views[k] = (left, right), each (R, t, twc, params8) as isInFrustumChecks takes them: GetPose() /
        GetCameraCenter() / mpCamera and GetRightPose() / GetRightCameraCenter() / mpCamera2.  map_points as FuseMapPoints; skip [K, n] or None.
        Returns (best_idx [K, 2, n] in the rig's numbering, best_dist [K, 2, n], projected [K, 2, n] or None)."""
        K = len(kfs)
        assert len(views) == K
        P, Nn = _f32(np.asarray(map_points["pos"]).reshape(-1, 3)), _f32(np.asarray(map_points["normal"]).reshape(-1, 3))
        mn, mx, d = _f32(map_points["min_dist"]), _f32(map_points["max_dist"]), _u8(map_points["desc"])
        n = len(P)
        sk = None if skip is None else _u8(np.asarray(skip).reshape(K, n))
        V = np.zeros(46 * max(K, 1), np.float32)
        for k, pair in enumerate(views):
            V[46 * k:46 * (k + 1)] = np.concatenate([np.asarray(x, np.float32).ravel() for cam in pair for x in cam])
        vp = C.c_void_p
        hs = (vp * max(K, 1))(*[kf._h.value if isinstance(kf._h, vp) else kf._h for kf in kfs])
        bi, bd = np.full((K, 2, n), -1, np.int32), np.full((K, 2, n), 256, np.int32)
        pr = np.zeros((K, 2, n), np.uint8) if want_projected else None
        check(self._L.orbx_keyframe_fuse_map_points_fisheye(self._h, K, hs, ptr(V), float(th), float(log_scale_factor), int(bool(strict_fp)), n, ptr(P),
                                                            ptr(Nn), ptr(mn), ptr(mx), ptr(d), ptr(sk), ptr(bi), ptr(bd), ptr(pr)),
              "orbx_keyframe_fuse_map_points_fisheye")
        return bi, bd, pr

    def FuseMapPoints(self, kfs, cams, poses, map_points: dict, th: float = 3.0, log_scale_factor: float = 0.0, skip=None,
                      strict_fp: bool = False, want_projected: bool = True):
        """The Fuse loop of LocalMapping::SearchInNeighbors in one call, projection included (orbx_keyframe_fuse_map_points).  cams[k] = orbx_camera
        fields (fx, fy, cx, cy, k1, k2, p1, p2, k3, bf), poses[k] = (Rcw, tcw, Ow) of key frame k; map_points: dict(pos [n, 3], normal [n, 3],
        min_dist, max_dist, desc [n, 32]); skip [K, n] = !pMP || isBad() || IsInKeyFrame(pKF_k) or None.
        Returns (best_idx [K, n], best_dist [K, n], projected [K, n] or None)."""
        from ._lib import Camera, FramePose
        K = len(kfs)
        assert len(cams) == K and len(poses) == K
        P, Nn = _f32(np.asarray(map_points["pos"]).reshape(-1, 3)), _f32(np.asarray(map_points["normal"]).reshape(-1, 3))
        mn, mx, d = _f32(map_points["min_dist"]), _f32(map_points["max_dist"]), _u8(map_points["desc"])
        n = len(P)
        sk = None if skip is None else _u8(np.asarray(skip).reshape(K, n))
        cs = (Camera * max(K, 1))(*[Camera(*[float(x) for x in c]) for c in cams])
        ps = (FramePose * max(K, 1))(*[FramePose.make(*p) for p in poses])
        vp = C.c_void_p
        hs = (vp * max(K, 1))(*[kf._h.value if isinstance(kf._h, vp) else kf._h for kf in kfs])
        bi, bd = np.full((K, n), -1, np.int32), np.full((K, n), 256, np.int32)
        pr = np.zeros((K, n), np.uint8) if want_projected else None
        check(self._L.orbx_keyframe_fuse_map_points(self._h, K, hs, cs, ps, float(th), float(log_scale_factor), int(bool(strict_fp)), n, ptr(P),
                                                    ptr(Nn), ptr(mn), ptr(mx), ptr(d), ptr(sk), ptr(bi), ptr(bd), ptr(pr)),
              "orbx_keyframe_fuse_map_points")
        return bi, bd, pr

    # ---- LoopClosing's Sim3 searches on resident key frames (ORBmatcher.cc:427-646, 1339-1455) ----
    def _sim3_args(self, kfs, cams, poses, map_points: dict, skip):
        from ._lib import Camera, FramePose
        K = len(kfs)
        assert len(cams) == K and len(poses) == K
        P, Nn = _f32(np.asarray(map_points["pos"]).reshape(-1, 3)), _f32(np.asarray(map_points["normal"]).reshape(-1, 3))
        mn, mx, d = _f32(map_points["min_dist"]), _f32(map_points["max_dist"]), _u8(map_points["desc"])
        n = len(P)
        sk = None if skip is None else _u8(np.asarray(skip).reshape(K, n))
        cs = (Camera * max(K, 1))(*[Camera(*[float(x) for x in c]) for c in cams])
        ps = (FramePose * max(K, 1))(*[FramePose.make(*p) for p in poses])
        return K, n, (P, Nn, mn, mx, d, sk), (self._kf_handles(kfs), cs, ps)

    def SearchByProjectionSim3KeyFrames(self, kfs, cams, poses, map_points: dict, th: float, ratio_hamming: float = 1.0, log_scale_factor: float = 0.0,
                                        projection_form: int = _lib.SIM3_PROJECT_CAMERA, skip=None, occupied=None, want_projected: bool = True,
                                        want_uv: bool = False):
        """SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (ORBmatcher.cc:427-532; projection_form SIM3_PROJECT_CAMERA) or its
        vpPointsKFs overload (:534-646; SIM3_PROJECT_INVZ) for K DeviceKeyFrames with one shared point set in one call
        (orbx_keyframe_search_by_projection_sim3).  cams[k] = orbx_camera fields, poses[k] = (Rcw, tcw, Ow) of Tcw = SE3f(Scw.rotationMatrix(),
        Scw.translation() / Scw.scale()); map_points as FuseMapPoints; skip [K, n] = isBad() || in spAlreadyFound of key frame k, or None; occupied:
        None, or per key frame a uint8[N_k] mask (vpMatched[i] != NULL) or None.  The key frames must share their image bounds.
        Returns (nmatches [K], match: K arrays of N_k map-point indices or -1, projected [K, n] or None, (proj_u, proj_v) [K, n] or None)."""
        K, n, (P, Nn, mn, mx, d, sk), (hs, cs, ps) = self._sim3_args(kfs, cams, poses, map_points, skip)
        keep, occ = self._flag_rows(occupied, K)
        match = [np.full(kf.count(), -1, np.int32) for kf in kfs]
        rows = (C.c_void_p * max(K, 1))(*[ptr(x) for x in match])
        nm = np.zeros(max(K, 1), np.int32)
        pr = np.zeros((K, n), np.uint8) if want_projected else None
        pu, pv = (np.zeros((K, n), np.float32), np.zeros((K, n), np.float32)) if want_uv else (None, None)
        check(self._L.orbx_keyframe_search_by_projection_sim3(self._h, K, hs, cs, ps, float(th), float(ratio_hamming), float(log_scale_factor),
                                                              int(projection_form), n, ptr(P), ptr(Nn), ptr(mn), ptr(mx), ptr(d), ptr(sk),
                                                              occ if occupied is not None else None, rows, ptr(nm), ptr(pr), ptr(pu), ptr(pv)),
              "orbx_keyframe_search_by_projection_sim3")
        del keep
        return nm[:K], match, pr, ((pu, pv) if want_uv else None)

    def FuseMapPointsSim3(self, kfs, cams, poses, map_points: dict, th: float = 3.0, log_scale_factor: float = 0.0, skip=None,
                          want_projected: bool = True):
        """The loop of LoopClosing::SearchAndFuse -- Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (ORBmatcher.cc:1339-1455) per key frame -- in one
        call, projection included (orbx_keyframe_fuse_map_points_sim3): the gate-less candidate search, no mvuRight.  Arguments as FuseMapPoints with
        poses[k] of Tcw = SE3f(Scw.rotationMatrix(), Scw.translation() / Scw.scale()); skip [K, n] = isBad() || in pKF_k->GetMapPoints(), or None.
        Returns (best_idx [K, n], best_dist [K, n], projected [K, n] or None)."""
        K, n, (P, Nn, mn, mx, d, sk), (hs, cs, ps) = self._sim3_args(kfs, cams, poses, map_points, skip)
        bi, bd = np.full((K, n), -1, np.int32), np.full((K, n), 256, np.int32)
        pr = np.zeros((K, n), np.uint8) if want_projected else None
        check(self._L.orbx_keyframe_fuse_map_points_sim3(self._h, K, hs, cs, ps, float(th), float(log_scale_factor), n, ptr(P), ptr(Nn), ptr(mn),
                                                         ptr(mx), ptr(d), ptr(sk), ptr(bi), ptr(bd), ptr(pr)),
              "orbx_keyframe_fuse_map_points_sim3")
        return bi, bd, pr

    def _sim3_fisheye_args(self, kfs, views, map_points: dict, skip):
        K = len(kfs)
        assert len(views) == K
        P, Nn = _f32(np.asarray(map_points["pos"]).reshape(-1, 3)), _f32(np.asarray(map_points["normal"]).reshape(-1, 3))
        mn, mx, d = _f32(map_points["min_dist"]), _f32(map_points["max_dist"]), _u8(map_points["desc"])
        n = len(P)
        sk = None if skip is None else _u8(np.asarray(skip).reshape(K, n))
        V = np.zeros(23 * max(K, 1), np.float32)   # ONE orbx_fisheye_view per key frame: the left camera's
        for k, cam in enumerate(views):
            V[23 * k:23 * (k + 1)] = np.concatenate([np.asarray(x, np.float32).ravel() for x in cam])
        return K, n, (P, Nn, mn, mx, d, sk), (self._kf_handles(kfs), V)

    def SearchByProjectionSim3KeyFramesFisheye(self, kfs, views, map_points: dict, th: float, ratio_hamming: float = 1.0,
                                               log_scale_factor: float = 0.0, projection_form: int = _lib.SIM3_PROJECT_CAMERA, skip=None, occupied=None,
                                               want_projected: bool = True, want_uv: bool = False):
        """SearchByProjectionSim3KeyFrames for K fisheye-stereo DeviceKeyFrames (orbx_keyframe_search_by_projection_sim3_fisheye): the members read the
        LEFT camera only.  views[k] = (R, t, twc, params8) of Tcw = SE3f(Scw.rotationMatrix(), Scw.translation() / Scw.scale()) with the left camera's
        parameters (SIM3_PROJECT_INVZ: params8[0..3] = pKF->fx, fy, cx, cy).  occupied: None, or per key frame a uint8[N_k] mask or None, N_k =
        N_left + N_right as vpMatched on a rig (entries from N_left on are not read).
        Returns (nmatches [K], match: K arrays of N_k map-point indices or -1 (always -1 from N_left on), projected [K, n] or None, (proj_u, proj_v)
        [K, n] or None)."""
        K, n, (P, Nn, mn, mx, d, sk), (hs, V) = self._sim3_fisheye_args(kfs, views, map_points, skip)
        keep, occ = self._flag_rows(occupied, K)
        match = [np.full(kf.count(), -1, np.int32) for kf in kfs]
        rows = (C.c_void_p * max(K, 1))(*[ptr(x) for x in match])
        nm = np.zeros(max(K, 1), np.int32)
        pr = np.zeros((K, n), np.uint8) if want_projected else None
        pu, pv = (np.zeros((K, n), np.float32), np.zeros((K, n), np.float32)) if want_uv else (None, None)
        check(self._L.orbx_keyframe_search_by_projection_sim3_fisheye(self._h, K, hs, ptr(V), float(th), float(ratio_hamming), float(log_scale_factor),
                                                                      int(projection_form), n, ptr(P), ptr(Nn), ptr(mn), ptr(mx), ptr(d), ptr(sk),
                                                                      occ if occupied is not None else None, rows, ptr(nm), ptr(pr), ptr(pu),
                                                                      ptr(pv)),
              "orbx_keyframe_search_by_projection_sim3_fisheye")
        del keep
        return nm[:K], match, pr, ((pu, pv) if want_uv else None)

    def FuseMapPointsSim3Fisheye(self, kfs, views, map_points: dict, th: float = 3.0, log_scale_factor: float = 0.0, skip=None,
                                 want_projected: bool = True):
        """FuseMapPointsSim3 for K fisheye-stereo DeviceKeyFrames (orbx_keyframe_fuse_map_points_sim3_fisheye): KannalaBrandt8::project of the left
        camera, the gate-less search of the left features.  views as SearchByProjectionSim3KeyFramesFisheye takes them.
        Returns (best_idx [K, n], always below N_left, best_dist [K, n], projected [K, n] or None)."""
        K, n, (P, Nn, mn, mx, d, sk), (hs, V) = self._sim3_fisheye_args(kfs, views, map_points, skip)
        bi, bd = np.full((K, n), -1, np.int32), np.full((K, n), 256, np.int32)
        pr = np.zeros((K, n), np.uint8) if want_projected else None
        check(self._L.orbx_keyframe_fuse_map_points_sim3_fisheye(self._h, K, hs, ptr(V), float(th), float(log_scale_factor), n, ptr(P), ptr(Nn), ptr(mn),
                                                                 ptr(mx), ptr(d), ptr(sk), ptr(bi), ptr(bd), ptr(pr)),
              "orbx_keyframe_fuse_map_points_sim3_fisheye")
        return bi, bd, pr

    # ---- the one-call searches with their map points resident (orbx_map): (map, ids) where the flat forms take the five arrays ----
    def SearchLocalPointsMap(self, F: DeviceFrame, cam, pose, log_scale_factor, cos_limit, map: DeviceMap, ids, eligible=None, has_obs=None,
                             th: float = 1.0, far_points: bool = False, th_far_points: float = 0.0, frame_occupied=None):
        """SearchLocalPoints with the map points named by id (orbx_frame_search_local_points_map): eligible / has_obs / in_view entry j belongs to
        ids[j] and frame_match holds POSITIONS in ids.  Returns (nmatches, frame_match[N], in_view[n_mp]) as SearchLocalPoints on the slots' rows."""
        from ._lib import Camera, FramePose
        i, el, ho, occ = _i32(ids), _u8(eligible), _u8(has_obs), _u8(frame_occupied)
        iv = np.zeros(len(i), np.uint8)
        fm = np.full(self._frame_rows(F, occ), -1, np.int32)
        c, p = Camera(*[float(x) for x in cam]), FramePose.make(*pose)
        n = check(self._L.orbx_frame_search_local_points_map(self._h, F._h, ptr(occ), C.byref(c), C.byref(p), float(log_scale_factor), float(cos_limit),
                                                             len(i), map._h, ptr(i), ptr(el), ptr(ho), float(th), self.mfNNratio,
                                                             int(bool(far_points)), float(th_far_points), ptr(iv), ptr(fm)),
                  "orbx_frame_search_local_points_map")
        return n, fm[:F.count()], iv

    def SearchLocalPointsFisheyeMap(self, F: DeviceFrame, views, log_scale_factor, cos_limit, map: DeviceMap, ids, eligible=None, has_obs=None,
                                    track_depth=None, th: float = 1.0, far_points: bool = False, th_far_points: float = 0.0, frame_occupied=None):
        """SearchLocalPointsFisheye with the map points named by id (orbx_frame_search_local_points_fisheye_map).
        Returns (nmatches, frame_match[N], in_view[2, n_mp])."""
        i, el, ho, td, occ = _i32(ids), _u8(eligible), _u8(has_obs), _f32(track_depth), _u8(frame_occupied)
        V = np.ascontiguousarray(np.concatenate([np.concatenate([np.asarray(x, np.float32).ravel() for x in v]) for v in views]), np.float32)
        assert V.size == 46, "views: left and right camera"
        iv = np.zeros((2, len(i)), np.uint8)
        fm = np.full(self._frame_rows(F, occ), -1, np.int32)
        n = check(self._L.orbx_frame_search_local_points_fisheye_map(self._h, F._h, ptr(occ), ptr(V), float(log_scale_factor), float(cos_limit), len(i),
                                                                     map._h, ptr(i), ptr(el), ptr(ho), ptr(td), float(th), self.mfNNratio,
                                                                     int(bool(far_points)), float(th_far_points), ptr(iv), ptr(fm)),
                  "orbx_frame_search_local_points_fisheye_map")
        return n, fm[:F.count()], iv

    def _pinhole_map_args(self, kfs, cams, poses, ids, skip):
        from ._lib import Camera, FramePose
        K, i = len(kfs), _i32(ids)
        assert len(cams) == K and len(poses) == K
        sk = None if skip is None else _u8(np.asarray(skip).reshape(K, len(i)))
        cs = (Camera * max(K, 1))(*[Camera(*[float(x) for x in c]) for c in cams])
        ps = (FramePose * max(K, 1))(*[FramePose.make(*p) for p in poses])
        return K, i, sk, self._kf_handles(kfs), cs, ps

    def _fisheye_map_args(self, kfs, views, ids, skip, per_kf: int):
        K, i = len(kfs), _i32(ids)
        assert len(views) == K
        sk = None if skip is None else _u8(np.asarray(skip).reshape(K, len(i)))
        V = np.zeros(23 * per_kf * max(K, 1), np.float32)   # per_kf orbx_fisheye_view records per key frame
        for k, v in enumerate(views):
            cams = v if per_kf == 2 else (v,)
            V[23 * per_kf * k:23 * per_kf * (k + 1)] = np.concatenate([np.asarray(x, np.float32).ravel() for cam in cams for x in cam])
        return K, i, sk, self._kf_handles(kfs), V

    def FuseMapPointsMap(self, kfs, cams, poses, map: DeviceMap, ids, th: float = 3.0, log_scale_factor: float = 0.0, skip=None,
                         strict_fp: bool = False, want_projected: bool = True):
        """FuseMapPoints with the map points named by id (orbx_keyframe_fuse_map_points_map).  Returns (best_idx [K, n], best_dist, projected)."""
        K, i, sk, hs, cs, ps = self._pinhole_map_args(kfs, cams, poses, ids, skip)
        n = len(i)
        bi, bd = np.full((K, n), -1, np.int32), np.full((K, n), 256, np.int32)
        pr = np.zeros((K, n), np.uint8) if want_projected else None
        check(self._L.orbx_keyframe_fuse_map_points_map(self._h, K, hs, cs, ps, float(th), float(log_scale_factor), int(bool(strict_fp)), n, map._h,
                                                        ptr(i), ptr(sk), ptr(bi), ptr(bd), ptr(pr)), "orbx_keyframe_fuse_map_points_map")
        return bi, bd, pr

    def FuseMapPointsFisheyeMap(self, kfs, views, map: DeviceMap, ids, th: float = 3.0, log_scale_factor: float = 0.0, skip=None,
                                strict_fp: bool = False, want_projected: bool = True):
        """FuseMapPointsFisheye with the map points named by id (orbx_keyframe_fuse_map_points_fisheye_map).
        Returns (best_idx [K, 2, n], best_dist [K, 2, n], projected [K, 2, n] or None)."""
        K, i, sk, hs, V = self._fisheye_map_args(kfs, views, ids, skip, 2)
        n = len(i)
        bi, bd = np.full((K, 2, n), -1, np.int32), np.full((K, 2, n), 256, np.int32)
        pr = np.zeros((K, 2, n), np.uint8) if want_projected else None
        check(self._L.orbx_keyframe_fuse_map_points_fisheye_map(self._h, K, hs, ptr(V), float(th), float(log_scale_factor), int(bool(strict_fp)), n,
                                                                map._h, ptr(i), ptr(sk), ptr(bi), ptr(bd), ptr(pr)),
              "orbx_keyframe_fuse_map_points_fisheye_map")
        return bi, bd, pr

    def FuseMapPointsSim3Map(self, kfs, cams, poses, map: DeviceMap, ids, th: float = 3.0, log_scale_factor: float = 0.0, skip=None,
                             want_projected: bool = True):
        """FuseMapPointsSim3 with the map points named by id (orbx_keyframe_fuse_map_points_sim3_map)."""
        K, i, sk, hs, cs, ps = self._pinhole_map_args(kfs, cams, poses, ids, skip)
        n = len(i)
        bi, bd = np.full((K, n), -1, np.int32), np.full((K, n), 256, np.int32)
        pr = np.zeros((K, n), np.uint8) if want_projected else None
        check(self._L.orbx_keyframe_fuse_map_points_sim3_map(self._h, K, hs, cs, ps, float(th), float(log_scale_factor), n, map._h, ptr(i), ptr(sk),
                                                             ptr(bi), ptr(bd), ptr(pr)), "orbx_keyframe_fuse_map_points_sim3_map")
        return bi, bd, pr

    def FuseMapPointsSim3FisheyeMap(self, kfs, views, map: DeviceMap, ids, th: float = 3.0, log_scale_factor: float = 0.0, skip=None,
                                    want_projected: bool = True):
        """FuseMapPointsSim3Fisheye with the map points named by id (orbx_keyframe_fuse_map_points_sim3_fisheye_map)."""
        K, i, sk, hs, V = self._fisheye_map_args(kfs, views, ids, skip, 1)
        n = len(i)
        bi, bd = np.full((K, n), -1, np.int32), np.full((K, n), 256, np.int32)
        pr = np.zeros((K, n), np.uint8) if want_projected else None
        check(self._L.orbx_keyframe_fuse_map_points_sim3_fisheye_map(self._h, K, hs, ptr(V), float(th), float(log_scale_factor), n, map._h, ptr(i),
                                                                     ptr(sk), ptr(bi), ptr(bd), ptr(pr)),
              "orbx_keyframe_fuse_map_points_sim3_fisheye_map")
        return bi, bd, pr

    def _sim3_search_outputs(self, kfs, K, n, occupied, want_projected, want_uv):
        keep, occ = self._flag_rows(occupied, K)
        match = [np.full(kf.count(), -1, np.int32) for kf in kfs]
        rows = (C.c_void_p * max(K, 1))(*[ptr(x) for x in match])
        nm = np.zeros(max(K, 1), np.int32)
        pr = np.zeros((K, n), np.uint8) if want_projected else None
        pu, pv = (np.zeros((K, n), np.float32), np.zeros((K, n), np.float32)) if want_uv else (None, None)
        return keep, (occ if occupied is not None else None), match, rows, nm, pr, pu, pv

    def SearchByProjectionSim3KeyFramesMap(self, kfs, cams, poses, map: DeviceMap, ids, th: float, ratio_hamming: float = 1.0,
                                           log_scale_factor: float = 0.0, projection_form: int = _lib.SIM3_PROJECT_CAMERA, skip=None, occupied=None,
                                           want_projected: bool = True, want_uv: bool = False):
        """SearchByProjectionSim3KeyFrames with the map points named by id (orbx_keyframe_search_by_projection_sim3_map): a match row holds
        POSITIONS in ids.  Returns (nmatches [K], match, projected [K, n] or None, (proj_u, proj_v) or None)."""
        K, i, sk, hs, cs, ps = self._pinhole_map_args(kfs, cams, poses, ids, skip)
        keep, occ, match, rows, nm, pr, pu, pv = self._sim3_search_outputs(kfs, K, len(i), occupied, want_projected, want_uv)
        check(self._L.orbx_keyframe_search_by_projection_sim3_map(self._h, K, hs, cs, ps, float(th), float(ratio_hamming), float(log_scale_factor),
                                                                  int(projection_form), len(i), map._h, ptr(i), ptr(sk), occ, rows, ptr(nm), ptr(pr),
                                                                  ptr(pu), ptr(pv)), "orbx_keyframe_search_by_projection_sim3_map")
        del keep
        return nm[:K], match, pr, ((pu, pv) if want_uv else None)

    def SearchByProjectionSim3KeyFramesFisheyeMap(self, kfs, views, map: DeviceMap, ids, th: float, ratio_hamming: float = 1.0,
                                                  log_scale_factor: float = 0.0, projection_form: int = _lib.SIM3_PROJECT_CAMERA, skip=None,
                                                  occupied=None, want_projected: bool = True, want_uv: bool = False):
        """SearchByProjectionSim3KeyFramesFisheye with the map points named by id (orbx_keyframe_search_by_projection_sim3_fisheye_map)."""
        K, i, sk, hs, V = self._fisheye_map_args(kfs, views, ids, skip, 1)
        keep, occ, match, rows, nm, pr, pu, pv = self._sim3_search_outputs(kfs, K, len(i), occupied, want_projected, want_uv)
        check(self._L.orbx_keyframe_search_by_projection_sim3_fisheye_map(self._h, K, hs, ptr(V), float(th), float(ratio_hamming),
                                                                          float(log_scale_factor), int(projection_form), len(i), map._h, ptr(i),
                                                                          ptr(sk), occ, rows, ptr(nm), ptr(pr), ptr(pu), ptr(pv)),
              "orbx_keyframe_search_by_projection_sim3_fisheye_map")
        del keep
        return nm[:K], match, pr, ((pu, pv) if want_uv else None)

    # ---- the Tracking thread's searches whose queries are another frame's map points, from map ids (k_track_project) ----
    def _track_outputs(self, Cur: DeviceFrame, n, occ, want_projected, want_uv):
        cm = np.full(self._frame_rows(Cur, occ), -1, np.int32)
        pr = np.zeros(n, np.uint8) if want_projected else None
        pu, pv = (np.zeros(n, np.float32), np.zeros(n, np.float32)) if want_uv else (None, None)
        return cm, pr, pu, pv

    def TrackLastFrame(self, Cur: DeviceFrame, Last: DeviceFrame, cam, pose, map: DeviceMap, ids, th: float, level_mode: int = 0, has_obs=None,
                       cur_occupied=None, want_projected: bool = True, want_uv: bool = False):
        """SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1676-1887) from map ids (orbx_frame_track_last_frame_map): ids[i] =
        the slot of LastFrame.mvpMapPoints[i] or -1 (none / outlier), has_obs[i] = Observations() > 0; cam / pose are the CURRENT frame's; the
        projection, the gates and the windows run on the device.  Returns (nmatches, cur_match [N], projected [n_ids] or None, (proj_u, proj_v) or
        None); cur_match[j] >= 0 is the LAST frame's feature index, -2 a slot the rotation check cleared."""
        from ._lib import Camera, FramePose
        i, ho, occ = _i32(ids), _u8(has_obs), _u8(cur_occupied)
        cm, pr, pu, pv = self._track_outputs(Cur, len(i), occ, want_projected, want_uv)
        c, p = Camera(*[float(x) for x in cam]), FramePose.make(*pose)
        n = check(self._L.orbx_frame_track_last_frame_map(self._h, Cur._h, Last._h, ptr(occ), C.byref(c), C.byref(p), map._h, len(i), ptr(i), ptr(ho),
                                                          float(th), int(level_mode), int(self.mbCheckOrientation), ptr(cm), ptr(pr), ptr(pu), ptr(pv)),
                  "orbx_frame_track_last_frame_map")
        return n, cm[:Cur.count()], pr, ((pu, pv) if want_uv else None)

    def SearchByProjectionKeyFrame(self, Cur: DeviceFrame, KF: DeviceKeyFrame, cam, pose, log_scale_factor: float, map: DeviceMap, ids, th: float,
                                   max_dist: float, check_orientation: bool = True, occupied=None, want_projected: bool = True,
                                   want_uv: bool = False):
        """SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1889-2010) from map ids
        (orbx_frame_search_by_projection_keyframe_map): ids[i] = the slot of pKF's map point i or -1 (none / bad / already found).
        Returns (nmatches, match [N], projected or None, (proj_u, proj_v) or None); match[j] >= 0 is the KEY FRAME's feature index."""
        from ._lib import Camera, FramePose
        i, occ = _i32(ids), _u8(occupied)
        cm, pr, pu, pv = self._track_outputs(Cur, len(i), occ, want_projected, want_uv)
        c, p = Camera(*[float(x) for x in cam]), FramePose.make(*pose)
        n = check(self._L.orbx_frame_search_by_projection_keyframe_map(self._h, Cur._h, ptr(occ), C.byref(c), C.byref(p), float(log_scale_factor),
                                                                       KF._h, map._h, len(i), ptr(i), float(th), float(max_dist),
                                                                       int(bool(check_orientation)), ptr(cm), ptr(pr), ptr(pu), ptr(pv)),
                  "orbx_frame_search_by_projection_keyframe_map")
        return n, cm[:Cur.count()], pr, ((pu, pv) if want_uv else None)

    @staticmethod
    def _left_view(view):
        V = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).ravel() for x in view]), np.float32)
        assert V.size == 23, "view: (R, t, twc, params8) of the left camera"
        return V

    def TrackLastFrameFisheye(self, Cur: DeviceFrame, Last: DeviceFrame, view, Trl, map: DeviceMap, ids, th: float, level_mode: int = 0, has_obs=None,
                              cur_occupied=None, want_projected: bool = True, want_uv: bool = False):
        """TrackLastFrame for a fisheye-stereo rig (orbx_frame_track_last_frame_fisheye_map): view = (R, t, twc, params8) of the CURRENT frame's left
        camera, Trl = (R [3, 3], t [3]) of GetRelativePoseTrl(); Last is a rig handle too and ids has N_left + N_right entries.  Returns as
        TrackLastFrame; cur_match holds N entries of both cameras."""
        i, ho, occ = _i32(ids), _u8(has_obs), _u8(cur_occupied)
        cm, pr, pu, pv = self._track_outputs(Cur, len(i), occ, want_projected, want_uv)
        V, R, t = self._left_view(view), _f32(np.asarray(Trl[0]).reshape(9)), _f32(np.asarray(Trl[1]).reshape(3))
        n = check(self._L.orbx_frame_track_last_frame_fisheye_map(self._h, Cur._h, Last._h, ptr(occ), ptr(V), ptr(R), ptr(t), map._h, len(i), ptr(i),
                                                                  ptr(ho), float(th), int(level_mode), int(self.mbCheckOrientation), ptr(cm), ptr(pr),
                                                                  ptr(pu), ptr(pv)), "orbx_frame_track_last_frame_fisheye_map")
        return n, cm[:Cur.count()], pr, ((pu, pv) if want_uv else None)

    def SearchByProjectionKeyFrameFisheye(self, Cur: DeviceFrame, KF: DeviceKeyFrame, view, log_scale_factor: float, map: DeviceMap, ids, th: float,
                                          max_dist: float, check_orientation: bool = True, occupied=None, want_projected: bool = True,
                                          want_uv: bool = False):
        """SearchByProjectionKeyFrame for a fisheye-stereo rig (orbx_frame_search_by_projection_keyframe_fisheye_map): the left camera only is
        searched; match holds N entries, the right camera's stay -1."""
        i, occ = _i32(ids), _u8(occupied)
        cm, pr, pu, pv = self._track_outputs(Cur, len(i), occ, want_projected, want_uv)
        V = self._left_view(view)
        n = check(self._L.orbx_frame_search_by_projection_keyframe_fisheye_map(self._h, Cur._h, ptr(occ), ptr(V), float(log_scale_factor), KF._h, map._h,
                                                                               len(i), ptr(i), float(th), float(max_dist), int(bool(check_orientation)),
                                                                               ptr(cm), ptr(pr), ptr(pu), ptr(pv)),
                  "orbx_frame_search_by_projection_keyframe_fisheye_map")
        return n, cm[:Cur.count()], pr, ((pu, pv) if want_uv else None)

    def DistinctiveDescriptorsKeyFramesToMap(self, kfs, set_ptr, obs_kf, obs_idx, map: DeviceMap, set_id):
        """DistinctiveDescriptorsKeyFrames with set s's winning row written into the descriptor of slot set_id[s] of the table
        (orbx_keyframe_distinctive_descriptors_to_map); an empty set leaves its slot as it is.  Returns best_obs[n_sets]."""
        sp, ok, oi, si = _i32(set_ptr), _i32(obs_kf), _i32(obs_idx), _i32(set_id)
        n_sets = len(sp) - 1
        assert n_sets >= 0 and len(ok) == len(oi) and len(si) == n_sets and (n_sets == 0 or sp[-1] <= len(ok))
        best = np.full(n_sets, -1, np.int32)
        check(self._L.orbx_keyframe_distinctive_descriptors_to_map(self._h, len(kfs), self._kf_handles(kfs), n_sets, ptr(sp), ptr(ok), ptr(oi),
                                                                   map._h, ptr(si), ptr(best)), "orbx_keyframe_distinctive_descriptors_to_map")
        return best

    # ---- MapPoint::UpdateNormalAndDepth on resident key frames (orbx_keyframe_update_normal_and_depth*) ----
    def _normal_depth_args(self, kfs, centers, centers_right, set_ptr, obs_kf, obs_idx, ref_obs):
        sp, ok, oi, ro = _i32(set_ptr), _i32(obs_kf), _i32(obs_idx), _i32(ref_obs)
        n_sets = len(sp) - 1
        ce = _f32(np.asarray(centers).reshape(-1, 3))
        cr = None if centers_right is None else _f32(np.asarray(centers_right).reshape(-1, 3))
        assert n_sets >= 0 and len(ok) == len(oi) and len(ro) == n_sets and (n_sets == 0 or sp[-1] <= len(ok))
        assert len(ce) == len(kfs) and (cr is None or len(cr) == len(kfs)), "one centre (and one right centre) per key frame"
        return n_sets, sp, ok, oi, ro, ce, cr

    def UpdateNormalAndDepthKeyFrames(self, kfs, centers, centers_right, set_ptr, obs_kf, obs_idx, ref_obs, pos):
        """MapPoint::UpdateNormalAndDepth for a batch of map points over DistinctiveDescriptorsKeyFrames' observation lists
        (orbx_keyframe_update_normal_and_depth): centers / centers_right [K, 3] = GetCameraCenter() / GetRightCameraCenter() (None without rigs),
        ref_obs[s] = the position inside set s of the reference key frame's observation, pos [n_sets, 3] = mWorldPos.  Returns
        (normal [n_sets, 3], min_dist, max_dist), the distances unscaled as the member leaves them; the rows of empty sets are zeros."""
        n_sets, sp, ok, oi, ro, ce, cr = self._normal_depth_args(kfs, centers, centers_right, set_ptr, obs_kf, obs_idx, ref_obs)
        P = _f32(np.asarray(pos).reshape(-1, 3))
        assert len(P) == n_sets
        normal, mn, mx = np.zeros((n_sets, 3), np.float32), np.zeros(n_sets, np.float32), np.zeros(n_sets, np.float32)
        check(self._L.orbx_keyframe_update_normal_and_depth(self._h, len(kfs), self._kf_handles(kfs), ptr(ce), ptr(cr), n_sets, ptr(sp), ptr(ok), ptr(oi),
                                                            ptr(ro), ptr(P), ptr(normal), ptr(mn), ptr(mx)), "orbx_keyframe_update_normal_and_depth")
        return normal, mn, mx

    def UpdateNormalAndDepthKeyFramesToMap(self, kfs, centers, centers_right, set_ptr, obs_kf, obs_idx, ref_obs, map: DeviceMap, set_id,
                                           want_outputs: bool = False):
        """The same with pos read from slot set_id[s] of the table and the results written into it (orbx_keyframe_update_normal_and_depth_to_map); an
        empty set leaves its slot as it is.  Returns (normal, min_dist, max_dist) with want_outputs, None otherwise -- the host's copies go stale then."""
        n_sets, sp, ok, oi, ro, ce, cr = self._normal_depth_args(kfs, centers, centers_right, set_ptr, obs_kf, obs_idx, ref_obs)
        si = _i32(set_id)
        assert len(si) == n_sets
        out = (np.zeros((n_sets, 3), np.float32), np.zeros(n_sets, np.float32), np.zeros(n_sets, np.float32)) if want_outputs else (None, None, None)
        check(self._L.orbx_keyframe_update_normal_and_depth_to_map(self._h, len(kfs), self._kf_handles(kfs), ptr(ce), ptr(cr), n_sets, ptr(sp), ptr(ok),
                                                                   ptr(oi), ptr(ro), map._h, ptr(si), ptr(out[0]), ptr(out[1]), ptr(out[2])),
              "orbx_keyframe_update_normal_and_depth_to_map")
        return out if want_outputs else None

    def RefreshMapPointsToMap(self, kfs, centers, centers_right, set_ptr, obs_kf, obs_idx, ref_obs, map: DeviceMap, set_id):
        """ComputeDistinctiveDescriptors and UpdateNormalAndDepth of a batch of map points in one call, straight into the table
        (orbx_keyframe_refresh_map_points_to_map): DistinctiveDescriptorsKeyFramesToMap followed by UpdateNormalAndDepthKeyFramesToMap, bit for bit,
        with one upload, one launch chain and one synchronisation.  Returns best_obs[n_sets]."""
        n_sets, sp, ok, oi, ro, ce, cr = self._normal_depth_args(kfs, centers, centers_right, set_ptr, obs_kf, obs_idx, ref_obs)
        si = _i32(set_id)
        assert len(si) == n_sets
        best = np.full(n_sets, -1, np.int32)
        check(self._L.orbx_keyframe_refresh_map_points_to_map(self._h, len(kfs), self._kf_handles(kfs), ptr(ce), ptr(cr), n_sets, ptr(sp), ptr(ok), ptr(oi),
                                                              ptr(ro), map._h, ptr(si), ptr(best)), "orbx_keyframe_refresh_map_points_to_map")
        return best

    # ---- SearchBySim3 (ORBmatcher.cc:1457-1674): two gate-less fuse searches + mutual agreement ----
    def SearchBySim3(self, KF1: FrameView, KF2: FrameView, side1: dict, side2: dict, th: float, already_matched1=None,
                     already_matched2=None, scale_factors1=None, scale_factors2=None):
        """side1: for every feature of KF1, its map point transformed by S21 and projected into KF2 — dict(valid, u, v, level,
        desc): valid[i] = the slot holds a good map point that survived the depth / image / distance gates of :1500-1527,
        (u, v) the projection, level = PredictScale(dist3D, pKF2), desc = pMP->GetDescriptor().  side2: the same for KF2's
        map points projected into KF1 (:1576-1645).  already_matched1/2 = vbAlreadyMatched1/2 (:1477-1490).  Search radius
        th * mvScaleFactors[level] of the key frame searched in.  Returns (nFound, match12[n1]) with match12[i1] = KF2 feature
        index (the reference stores vpMapPoints2[idx2]) or -1; slots the caller had matched already are left at -1."""
        sf1 = _f32(KF1.scale_factors if scale_factors1 is None else scale_factors1)
        sf2 = _f32(KF2.scale_factors if scale_factors2 is None else scale_factors2)

        def one_way(side, target: FrameView, sf, done):
            lv = _i32(side["level"])
            ok = _u8(side["valid"]) == 1
            if done is not None:
                ok &= _u8(done) == 0
            q = dict(u=side["u"], v=side["v"], ur=np.zeros(len(lv), np.float32), r=(np.float32(th) * sf[lv]).astype(np.float32),
                     level=lv, desc=side["desc"])
            bi, bd = self.FuseSearch(target, q, None)
            return np.where(ok & (bd <= 100), bi, -1)          # bestDist <= TH_HIGH (:1569, :1656)
        m1 = one_way(side1, KF2, sf2, already_matched1)
        m2 = one_way(side2, KF1, sf1, already_matched2)
        back = np.where(m1 >= 0, m2[np.maximum(m1, 0)], -2)
        match12 = np.where(back == np.arange(len(m1)), m1, -1).astype(np.int32)   # :1662-1675 agreement check
        return int((match12 >= 0).sum()), match12
