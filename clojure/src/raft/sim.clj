(ns raft.sim
  "Batched MI355X simulation of raft.core's node loop (src/raft/core.clj:176-203 of the reference)
  through libraftsim.so, the C ABI of include/raftsim.h (ABI version 2). One handle simulates
  n-clusters independent clusters of `nodes` nodes each on `n-devices` GPUs; a node is the map
  init-node builds (core.clj:31-38) and every `wait` iteration of every node happens inside step!.
  Semantics: SIM_SPEC.md. JNA, because Clojure 1.6 predates Panama (JDK 22)."
  (:import [com.sun.jna NativeLibrary Memory Pointer Function]
           [com.sun.jna.ptr PointerByReference]))

(def ^:private lib (delay (NativeLibrary/getInstance "raftsim")))

(defn- f ^Function [fname] (.getFunction ^NativeLibrary @lib fname))

(defn- last-error [] (.getString ^Pointer (.invokePointer (f "raft_sim_last_error") (object-array [])) 0))

(defn- check
  "raft_sim_* calls return 0 or a negative errno (include/raftsim.h); never throw across the ABI."
  [rc]
  (when (neg? rc) (throw (ex-info (last-error) {:rc rc})))
  rc)

(defn- call [fname & args] (check (.invokeInt (f fname) (object-array args))))

(def abi-version 2)

;; raft_sim_config_t (120 bytes): u32 fields, the u64 seed at 24, i32 device and n_devices
(def config-offsets
  {:n-clusters 0 :cluster-offset 4 :nodes 8 :log-cap 12 :arena-cap 16 :inbox-cap 20 :seed 24
   :hb 32 :el-base 36 :el-span 40 :drop-ppm 44 :dup-ppm 48 :dmin 52 :dmax 56 :part-ppm 60
   :part-epoch 64 :client-ppm 68 :variant-flags 72 :device 76 :ticks-per-launch 80
   :commit-stream-cap 84 :trace-cap 88 :trace-entry-cap 92 :schedule 96 :client-period 100
   :client-burst 104 :client-redirects 108 :n-devices 112})
(def config-size 120)

;; raft_node_t (136 bytes)
(def node-offsets
  {:role 0 :voted-for 1 :leader-id 2 :fault 3 :entries-is-seq 4 :ls-present 5 :votes 6 :ls-keys 8
   :current-term 12 :commit-index 16 :log-len 20 :deadline 24 :next-index 28 :match-index 64
   :last-led-term 100 :arena-base 104 :arena-frontier 108 :req-count 112 :res-count 116
   :commit-count 120 :trace-hash 128})
(def node-size 136)

;; raft_counters_t (248 bytes): node_ticks, first_violation_tick, 28 sums, payload_max
(def counter-names
  [:ev-rv :ev-ae :ev-cs :ev-vr :ev-ar :ev-timeout :ev-heartbeat :leaders :sent :delivered :dropped
   :partitioned :duplicated :overflow :to-halted :client-injected :halt-ioobe :halt-npe :halt-cce
   :halt-overflow :entries-appended :entries-applied :payload-evicted :viol-election :viol-log
   :viol-complete :redirects :client-abandoned])
(def counters-size 248)

(def ^:private states [:follower :candidate :leader :follwer])   ; :follwer is core.clj:76's typo
(def ^:private halts {1 :index-out-of-bounds 2 :null-pointer 3 :class-cast 4 :log-capacity})

(defn create
  "Like (component/start (raft-system id cluster)) (core.clj:23-29,201) for every node of
  n-clusters clusters. cfg keys: config-offsets; absent keys keep raft_sim_default_config."
  [cfg]
  (let [m (Memory. config-size)]
    (.invokeVoid (f "raft_sim_default_config") (object-array [m]))
    (doseq [[k v] cfg :let [off (config-offsets k)]]
      (when-not off (throw (ex-info "unknown config key" {:key k})))
      (if (= k :seed) (.setLong m off (long v)) (.setInt m off (unchecked-int v))))
    (let [out (PointerByReference.)]
      (call "raft_sim_create" m out)
      {:ptr (.getValue out) :nodes (int (:nodes cfg 5))})))

(defn step!
  "(loop [node ...] (recur (wait system node))) of core.clj:202-203, `ticks` times, for all nodes."
  [sim ticks]
  (call "raft_sim_step" (:ptr sim) (int ticks))
  sim)

(defn tick [sim] (.invokeLong (f "raft_sim_tick") (object-array [(:ptr sim)])))

(defn set-tick!
  "Resume at `t` after restoring state through the write calls (deadlines are absolute ticks)."
  [sim t]
  (call "raft_sim_set_tick" (:ptr sim) (long t))
  sim)

(defn nodes
  "The node maps of cluster c, shaped like init-node (core.clj:31-38), plus :halted."
  [sim c]
  (let [n (:nodes sim)
        m (Memory. (* node-size n))
        ids (fn [mask] (set (filter #(bit-test mask %) (range 1 (inc n)))))]
    (call "raft_sim_read_nodes" (:ptr sim) (int c) (int 1) m)
    (vec (for [i (range n)
               :let [b (* i node-size)
                     at (fn [k] (+ b (node-offsets k)))
                     ls-keys (ids (.getShort m (at :ls-keys)))
                     peer-map (fn [k] (into {} (for [p ls-keys]
                                                 [p (.getInt m (+ (at k) (* 4 (dec p))))])))]]
           {:id (inc i)
            :state (states (.getByte m (at :role)))
            :current-term (.getInt m (at :current-term))
            :voted-for (let [v (.getByte m (at :voted-for))] (when (pos? v) v))
            :leader-id (let [v (.getByte m (at :leader-id))] (when (pos? v) v))
            :leader-state (when (pos? (.getByte m (at :ls-present)))
                            {:next-index (peer-map :next-index)
                             :match-index (peer-map :match-index)})
            :votes (ids (.getShort m (at :votes)))
            :halted (halts (.getByte m (at :fault)))}))))

(defn log-entries
  "The Log atom's :entries of node `id` of cluster c (log.clj:33-34), as {:term t :val v} maps."
  [sim c id]
  (let [node (Memory. (* node-size (:nodes sim)))
        _ (call "raft_sim_read_nodes" (:ptr sim) (int c) (int 1) node)
        b (* (dec id) node-size)
        base (.getInt node (+ b (node-offsets :arena-base)))
        len (.getInt node (+ b (node-offsets :log-len)))
        cap (call "raft_sim_read_arena" (:ptr sim) (int c) (int id) nil (int 0))
        ar (Memory. (* 8 cap))]
    (call "raft_sim_read_arena" (:ptr sim) (int c) (int id) ar (int cap))
    (vec (for [i (range len) :let [s (* 8 (mod (+ base i) cap))]]
           {:term (.getInt ar s) :val (.getInt ar (+ s 4))}))))

(defn commit-log
  "What apply-entries! wrote to node_<id>.log (log.clj:16-18,69-76), newest commit_stream_cap."
  [sim c id cap]
  (let [m (Memory. (* 4 (max 1 cap)))
        n (call "raft_sim_read_commit_stream" (:ptr sim) (int c) (int id) m (int cap))]
    (vec (for [i (range n)] (.getInt m (* 4 i))))))

(defn counters
  "Counters of every cluster of the handle, reduced over its devices (SUM; first violation MIN;
  payload maximum MAX)."
  [sim]
  (let [m (Memory. counters-size)]
    (call "raft_sim_read_counters" (:ptr sim) m)
    (merge (zipmap counter-names (for [i (range (count counter-names))] (.getLong m (+ 16 (* 8 i)))))
           {:node-ticks (.getLong m 0)
            :first-violation-tick (let [v (.getLong m 8)] (when-not (= v -1) v))
            :payload-max (.getLong m 240)})))

;; raft_violation_t (24 bytes): cluster, first_tick, count[3] (election, log matching, leader
;; completeness), kinds. No reference counterpart: the per-cluster record behind the counters.
(def violation-size 24)
(def ^:private viol-kinds {:election 1 :log 2 :complete 4})

(defn violations
  "The clusters the checker counted a violation for, in ascending cluster order: {:total n
  :records [...]}, a cluster matching when it has a violation of one of `kinds` (a subset of
  #{:election :log :complete}) and its first violation tick lies in [t-lo, t-hi). At most `cap`
  records are copied (cap 0: the total alone); the selection runs on the device."
  [sim kinds t-lo t-hi cap]
  (let [mask (reduce bit-or 0 (map viol-kinds kinds))
        m (Memory. (* violation-size (max 1 cap)))
        total (.invokeLong (f "raft_viol_read")
                           (object-array [(:ptr sim) (int mask) (long t-lo) (long t-hi)
                                          (when (pos? cap) m) (int cap)]))]
    (when (neg? total) (throw (ex-info (last-error) {:rc total})))
    {:total total
     :records (vec (for [i (range (min total cap)) :let [b (* i violation-size)]]
                     {:cluster (.getInt m b)
                      :first-tick (.getInt m (+ b 4))
                      :election (.getInt m (+ b 8))
                      :log (.getInt m (+ b 12))
                      :complete (.getInt m (+ b 16))
                      :kinds (set (for [[k bit] viol-kinds
                                        :when (pos? (bit-and bit (.getInt m (+ b 20))))] k))}))}))

(defn clear-violations!
  "Forget every cluster's violation record (state, digests and counters are unchanged)."
  [sim]
  (call "raft_viol_clear" (:ptr sim))
  sim)

;; raft_census_t (464 bytes, 58 u64): clusters 0, nodes 8, by_class[16] 16, leaders_hist[10] 144,
;; live_hist[10] 224, role_nodes[4] 304, fault_nodes[5] 336, then eleven scalars from 376.
;; No reference counterpart: what state the clusters are in now, counted on the device.
(def census-size 464)
(def cluster-classes
  {:no-leader 1 :one-leader 2 :multi-leader 4 :halted 8 :no-quorum 16 :same-term-leaders 32
   :log-full 64 :candidate 128 :settled 256})
(def ^:private class-order
  [:no-leader :one-leader :multi-leader :halted :no-quorum :same-term-leaders :log-full :candidate
   :settled])
(def ^:private census-scalars
  [:term-min :term-max :term-sum :commit-max :commit-sum :len-max :len-sum :req-queued :res-queued
   :hwm-max :hwm-sum])

(defn census
  "The census of every cluster of the handle (raft_census_read): :by-class maps each class of
  cluster-classes to its number of clusters, :leaders-hist / :live-hist count the clusters with
  exactly i live leaders / live nodes, :role-nodes live nodes by :state, :fault-nodes all nodes by
  halt code; the rest are sums and extrema over all nodes and clusters."
  [sim]
  (let [m (Memory. census-size)
        n (inc (:nodes sim))
        u64s (fn [off cnt] (vec (for [i (range cnt)] (.getLong m (+ off (* 8 i))))))]
    (call "raft_census_read" (:ptr sim) m)
    (merge {:clusters (.getLong m 0)
            :nodes (.getLong m 8)
            :by-class (zipmap class-order (u64s 16 9))
            :leaders-hist (u64s 144 n)
            :live-hist (u64s 224 n)
            :role-nodes (u64s 304 4)
            :fault-nodes (u64s 336 5)}
           (zipmap census-scalars (u64s 376 11)))))

;; raft_cluster_state_t (32 bytes): cluster 0, classes 4, leaders 8 and halted 10 (u16 masks, bit i
;; = id i), term_max 12, term_min 16, commit_max 20, len_max 24, queued 28.
(def cluster-state-size 32)

(defn select-clusters
  "The clusters in given state classes, in ascending cluster order (raft_census_select): {:total n
  :records [...]}. A cluster matches when it is in one of the classes `any` (empty: no such
  condition), in all of `all` and in none of `none` (subsets of the keys of cluster-classes). At
  most `cap` records are copied (cap 0: the total alone); the selection runs on the device."
  [sim any all none cap]
  (let [mask (fn [ks] (int (reduce bit-or 0 (map cluster-classes ks))))
        m (Memory. (* cluster-state-size (max 1 cap)))
        total (.invokeLong (f "raft_census_select")
                           (object-array [(:ptr sim) (mask any) (mask all) (mask none)
                                          (when (pos? cap) m) (int cap)]))
        ids (fn [bits] (set (filter #(bit-test bits %) (range 1 (inc (:nodes sim))))))]
    (when (neg? total) (throw (ex-info (last-error) {:rc total})))
    {:total total
     :records (vec (for [i (range (min total cap)) :let [b (* i cluster-state-size)]]
                     {:cluster (.getInt m b)
                      :classes (set (for [[k bit] cluster-classes
                                          :when (pos? (bit-and bit (.getInt m (+ b 4))))] k))
                      :leaders (ids (.getShort m (+ b 8)))
                      :halted (ids (.getShort m (+ b 10)))
                      :term-max (.getInt m (+ b 12))
                      :term-min (.getInt m (+ b 16))
                      :commit-max (.getInt m (+ b 20))
                      :len-max (.getInt m (+ b 24))
                      :queued (.getInt m (+ b 28))}))}))

;; raft_audit_t (136 bytes, 17 u64): clusters 0, by_class[8] 8, then eight scalars from 72.
;; No reference counterpart: whether the nodes' logs agree as they stand, read on the device.
(def audit-size 136)
(def audit-classes
  {:diverged 1 :commit-diverged 2 :match-broken 4 :term-order 8 :identical 16})
(def ^:private audit-class-order
  [:diverged :commit-diverged :match-broken :term-order :identical])
(def ^:private audit-scalars
  [:entries :agree-sum :agree-min :agree-max :diverged-nodes :commit-diverged-nodes
   :diverge-index-min :commit-diverge-index-min])

(defn audit
  "The log audit of every cluster of the handle (raft_audit_read): :by-class maps each class of
  audit-classes to its number of clusters, :entries is the sum of all log lengths, :agree-* the
  common prefix of a cluster's logs over the clusters, :*-nodes the nodes in a diverging pair and
  :*-index-min the first diverging position anywhere (-1, UINT64_MAX, when there is none)."
  [sim]
  (let [m (Memory. audit-size)
        a64s (fn [off cnt] (vec (for [i (range cnt)] (.getLong m (+ off (* 8 i))))))]
    (call "raft_audit_read" (:ptr sim) m)
    (merge {:clusters (.getLong m 0)
            :by-class (zipmap audit-class-order (a64s 8 5))}
           (zipmap audit-scalars (a64s 72 8)))))

;; raft_audit_record_t (32 bytes): cluster 0, classes 4, agree_len 8, diverge_index 12,
;; commit_diverge_index 16, order_index 20 (an index of -1, UINT32_MAX: none), diverged 24 and
;; commit_diverged 26 (u16 masks, bit i = id i), len_min 28.
(def audit-record-size 32)

(defn audit-select
  "The clusters in given audit classes, in ascending cluster order (raft_audit_select): {:total n
  :records [...]}, with the predicate of select-clusters over the keys of audit-classes. At most
  `cap` records are copied (cap 0: the total alone); the selection runs on the device."
  [sim any all none cap]
  (let [mask (fn [ks] (int (reduce bit-or 0 (map audit-classes ks))))
        m (Memory. (* audit-record-size (max 1 cap)))
        total (.invokeLong (f "raft_audit_select")
                           (object-array [(:ptr sim) (mask any) (mask all) (mask none)
                                          (when (pos? cap) m) (int cap)]))
        ids (fn [bits] (set (filter #(bit-test bits %) (range 1 (inc (:nodes sim))))))]
    (when (neg? total) (throw (ex-info (last-error) {:rc total})))
    {:total total
     :records (vec (for [i (range (min total cap)) :let [r (* i audit-record-size)]]
                     {:cluster (.getInt m r)
                      :classes (set (for [[k bit] audit-classes
                                          :when (pos? (bit-and bit (.getInt m (+ r 4))))] k))
                      :agree-len (.getInt m (+ r 8))
                      :diverge-index (.getInt m (+ r 12))
                      :commit-diverge-index (.getInt m (+ r 16))
                      :order-index (.getInt m (+ r 20))
                      :diverged (ids (.getShort m (+ r 24)))
                      :commit-diverged (ids (.getShort m (+ r 26)))
                      :len-min (.getInt m (+ r 28))}))}))

;; raft_gather_layout_t (104 bytes, 13 u64): stride 0, off[6] 8, size[6] 56. No reference
;; counterpart: the full state of a list of clusters, packed on the device.
(def gather-layout-size 104)
(def gather-parts
  {:cluster 1 :nodes 2 :queues 4 :logs 8 :arenas 16 :streams 32})
(def ^:private gather-part-order [:cluster :nodes :queues :logs :arenas :streams])

(defn gather-layout
  "Where the parts (a subset of the keys of gather-parts) stand in a cluster's record
  (raft_gather_layout): {:stride bytes, part {:off o :size s}} for the parts asked for."
  [sim parts]
  (let [m (Memory. gather-layout-size)
        mask (int (reduce bit-or 0 (map gather-parts parts)))]
    (call "raft_gather_layout" (:ptr sim) mask m)
    (into {:stride (.getLong m 0)}
          (for [[b k] (map-indexed vector gather-part-order)
                :let [off (.getLong m (+ 8 (* 8 b)))]
                :when (not= off -1)]                    ; UINT64_MAX: not asked for
            [k {:off off :size (.getLong m (+ 56 (* 8 b)))}]))))

(defn gather
  "The full state of the clusters `cs` (handle-local indices, any order) packed on the device
  (raft_gather_read): {:layout (gather-layout sim parts) :buffer m}, record i of the Memory m
  being cluster (nth cs i) at byte (* i stride). :nodes carries the counts of the other parts."
  [sim cs parts]
  (let [layout (gather-layout sim parts)
        n (count cs)
        bytes (* n (:stride layout))
        idx (Memory. (* 4 (max 1 n)))
        m (Memory. (max 1 bytes))
        mask (int (reduce bit-or 0 (map gather-parts parts)))]
    (doseq [[i c] (map-indexed vector cs)] (.setInt idx (* 4 i) (unchecked-int c)))
    (let [rc (.invokeLong (f "raft_gather_read")
                          (object-array [(:ptr sim) idx (int n) mask m (long bytes)]))]
      (when (neg? rc) (throw (ex-info (last-error) {:rc rc})))
      {:layout layout :buffer m})))

(defn scatter
  "The way back (raft_scatter_write): record (nth rs i) of `buffer`, a Memory of n-records records
  of `parts` as gather returns it, becomes cluster (nth cs i) of sim; rs nil takes record i. A
  record may be named any number of times (one state, many futures), a cluster once. `parts` must
  hold :cluster :nodes :queues :arenas, and :streams when the handle keeps commit streams. Does not
  set the clock (set-tick!). Returns the number of clusters written."
  [sim cs rs parts buffer n-records]
  (let [n (count cs)
        ints (fn [xs] (let [m (Memory. (* 4 (max 1 n)))]
                        (doseq [[i x] (map-indexed vector xs)] (.setInt m (* 4 i) (unchecked-int x)))
                        m))
        mask (int (reduce bit-or 0 (map gather-parts parts)))
        rc (.invokeLong (f "raft_scatter_write")
                        (object-array [(:ptr sim) (ints cs) (when rs (ints rs)) (int n) mask buffer
                                       (int n-records)]))]
    (when (neg? rc) (throw (ex-info (last-error) {:rc rc})))
    rc))

(defn clone
  "Cluster state copied on the device (raft_clone_write): cluster (nth ts i) of `dst` becomes the
  state of cluster (nth ss i) of `src`, which may be dst, as a scatter of a gather would leave it,
  with no pack in host memory. A source may be named any number of times (one state, many futures),
  a target once, and within one handle no cluster may be both. The handles must agree in nodes,
  inbox-cap, log-cap, arena-cap and commit-stream-cap and live on one GPU. Does not set a clock
  (set-tick!). Returns the number of clusters written."
  [dst ts src ss]
  (let [n (count ts)
        _ (when (not= n (count ss))
            (throw (ex-info "clone: as many sources as targets" {:targets n :sources (count ss)})))
        ints (fn [xs] (let [m (Memory. (* 4 (max 1 n)))]
                        (doseq [[i x] (map-indexed vector xs)] (.setInt m (* 4 i) (unchecked-int x)))
                        m))
        rc (.invokeLong (f "raft_clone_write")
                        (object-array [(:ptr dst) (ints ts) (:ptr src) (ints ss) (int n)]))]
    (when (neg? rc) (throw (ex-info (last-error) {:rc rc})))
    rc))

(def restart-modes {:amnesia 0 :durable 1})

(defn restart
  "Nodes started again on the device at the handle's tick (raft_restart_write; SIM_SPEC §4a): node id
  j of cluster (nth cs i) is restarted where bit j of (nth masks i) is set (as :votes). `mode` is
  :amnesia (the reference's JVM started again: init-node and a fresh log, nothing read from disk) or
  :durable (current-term, voted-for and the log survive: Raft's Figure 2). Both empty the node's
  queues and re-arm its election timer from the current tick. A cluster may be named once. Returns
  the number of nodes restarted."
  [sim cs masks mode]
  (let [n (count cs)
        _ (when (not= n (count masks))
            (throw (ex-info "restart: as many masks as clusters" {:clusters n :masks (count masks)})))
        ints (Memory. (* 4 (max 1 n)))
        shorts (Memory. (* 2 (max 1 n)))
        _ (doseq [[i c] (map-indexed vector cs)] (.setInt ints (* 4 i) (unchecked-int c)))
        _ (doseq [[i m] (map-indexed vector masks)] (.setShort shorts (* 2 i) (unchecked-short m)))
        rc (.invokeLong (f "raft_restart_write")
                        (object-array [(:ptr sim) ints shorts (int n) (int (restart-modes mode mode))]))]
    (when (neg? rc) (throw (ex-info (last-error) {:rc rc})))
    rc))

(defn restart-where
  "Every node of the handle whose fault code f has bit f set in `fault-mask` (1..31; bit 0 = the
  running nodes, 1 IOOBE, 2 NPE, 3 CCE, 4 OVERFLOW) started again, found and counted on the device
  in one pass (raft_restart_where). `mode` as in restart. Returns the number of nodes restarted."
  [sim fault-mask mode]
  (let [rc (.invokeLong (f "raft_restart_where")
                        (object-array [(:ptr sim) (int fault-mask) (int (restart-modes mode mode))]))]
    (when (neg? rc) (throw (ex-info (last-error) {:rc rc})))
    rc))

(defn digest
  "Per-cluster FNV-1a-64 of the canonical state (SIM_SPEC §6) for clusters [c0, c0+nc)."
  [sim c0 nc]
  (let [m (Memory. (* 8 nc))]
    (call "raft_sim_digest" (:ptr sim) (int c0) (int nc) m)
    (vec (for [i (range nc)] (.getLong m (* 8 i))))))

(defn destroy! [sim]
  (.invokeVoid (f "raft_sim_destroy") (object-array [(:ptr sim)])))
