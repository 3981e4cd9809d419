%% ra_gpu_batch -- Erlang side of the NIF (ra_amd/csrc/ra_gpu_batch_nif.c) plus the helpers the
%% gen_statem shell needs to route ra_server transitions through the GPU engine.
%%
%% NOT COMPILED OR RUN IN THIS REPOSITORY'S ENVIRONMENT (no Erlang/OTP here); it documents the
%% reference-side binding a maintainer would add.  INTEGRATION.md walks through it.
%%
%% Records cross the NIF boundary as binaries with the C layout of include/ra_gpu_batch.h:
%%   rgb_msg      64 bytes, little endian:
%%     server:32, kind:8, from:8, flags:8, gap:8, term:64, a:64, b:64, c:64,
%%     n_entries:32, n_run0:32, run0_term:64, run1_term:64
%%   rgb_decision 64 bytes:
%%     server:32, role:8, reply_to:8, n_rpcs:8, kind:8, flags:32, invariant:16, heartbeat_to:8, cancel_backoff:8,
%%     reply_term:64, reply_next_index:64, reply_last_index:64, reply_last_term:64,
%%     commit_index:64, last_applied:64
-module(ra_gpu_batch).

-export([init/0, open/4, register_groups/3, upload_state/3, download_state/3, register_owner/4, unregister_owner/2, owner_slots/1, fan_back_stats/1, route/2,
         submit/3, submit/4, submit_raw/4, collect/1, start_collector/2, stop_collector/1, snapshot/2, wal_checksums/3,
         comm_unique_id/0, comm_init/4, allgather_leaderboard/2, node_leaderboard/3]).
-export([wal_batch_checksums/2, wal_frame/4, wal_recover_check/2, wal_frame_batch/3, wal_recover/2]).
-export([crc32s/3, crc32_stream/3, segment_build/5, segment_image/4]).
-export([segment_info/4, segment_compact/6, segment_compact_group/4]).
-export([segment_compact_plan/7, segment_compact_groups/7, major_compaction_batch/4]).
-export([segment_flush/7, segment_flush_batch/5]).
-export([wal_batch/6, wal_handle_batch/5]).
-export([segment_read/5, segment_read_plan/3, segment_term_query_batch/2]).
-export([crc32_spans/3, snapshot_build/3, snapshot_validate/3, snapshot_images/2, snapshot_recover_batch/2, accept_chunks/2]).
-export([encode_msg/3, encode_msgs/1, decode_decision/1, decision_to_effects/3]).

-include_lib("ra/src/ra.hrl").

-on_load(init/0).

-define(MSG_AER, 1).
-define(MSG_AER_REPLY, 2).
-define(MSG_REQUEST_VOTE, 3).
-define(MSG_VOTE_RESULT, 4).
-define(MSG_WRITTEN, 5).
-define(MSG_PIPELINE_RPCS, 6).
-define(MSG_APPEND, 7).
-define(MSG_AWAIT_TIMEOUT, 8).
-define(MSG_ELECTION_TIMEOUT, 9).
-define(MSG_PRE_VOTE_RPC, 10).
-define(MSG_PRE_VOTE_RESULT, 11).
-define(MSG_SNAPSHOT_WRITTEN, 12).
-define(MSG_HEARTBEAT_RPC, 13).
-define(MSG_HEARTBEAT_REPLY, 14).
-define(MSG_CONSISTENT_QUERY, 15).
-define(MSG_TRANSFER_LEADERSHIP, 16).
-define(NONE, 255).
-define(UNDEF, 16#FFFFFFFFFFFFFFFF).

-define(F_REPLY, 1).
-define(F_REPLY_SUCCESS, 2).
-define(F_REPLY_VOTE, 4).
-define(F_PERSIST, 8).
-define(F_LEADER_MSG, 16).
-define(F_APPLIED, 64).
-define(F_AUX_EVAL, 128).
-define(F_PIPELINE, 1024).
-define(F_INVARIANT, 32768).
-define(F_REPLY_PRE_VOTE, 262144).
-define(F_RESEND_PENDING, 4194304).
-define(F_REPLY_HEARTBEAT, 8388608).
-define(F_SEND_HEARTBEATS, 16777216).
-define(F_QUERY_QUORUM, 33554432).
-define(F_QUERY_APPLY, 67108864).
-define(F_CANCEL_SNAPSHOT_RETRY, 134217728).
-define(F_TRANSFER_LEADERSHIP, 536870912).
-define(F_CALL_REPLY, 1073741824).
%% reply_next_index under F_CALL_REPLY (RGB_CALL_* of the header)
-define(CALL_OK, 0).
-define(CALL_ALREADY_LEADER, 1).
-define(CALL_UNKNOWN_MEMBER, 2).
-define(CALL_NON_VOTER, 3).
-define(CALL_NOT_UP_TO_DATE, 4).
-define(CALL_UNSUPPORTED, 5).

init() ->
    erlang:load_nif(filename:join(code:priv_dir(ra), "ra_gpu_batch_nif"), 0).

open(_Device, _MaxRuns, _RingSlots, _RingCapacity) -> erlang:nif_error(not_loaded).
register_groups(_Ctx, _NGroups, _NMembers) -> erlang:nif_error(not_loaded).
upload_state(_Ctx, _First, _Bin) -> erlang:nif_error(not_loaded).
download_state(_Ctx, _First, _N) -> erlang:nif_error(not_loaded).
%% route(GroupUId, NContexts) -> 0..NContexts-1: the context (one per GPU, one open/4 each) that owns a Raft group:
%% splitmix64(GroupUId) rem NContexts, the partition of SURVEY.md section 8(e).  GroupUId = any stable 64-bit id of
%% the cluster (e.g. erlang:phash2 is NOT stable across nodes; use the integer kept beside the ra_directory entry).
route(_GroupUId, _NContexts) -> erlang:nif_error(not_loaded).
%% register_owner(Ctx, FirstServer, N, Pid): the collector thread sends every decision of servers
%% [FirstServer, FirstServer+N) to Pid as {ra_gpu_batch, Tick, NDecisions, DecisionsBin, RpcsBin} (only that
%% process's decisions, submission order; rpc msg_index = position inside DecisionsBin).  A ra_server_proc
%% registers itself for its one server in init/1; unregistered servers go to the start_collector/2 pid.
register_owner(_Ctx, _FirstServer, _N, _Pid) -> erlang:nif_error(not_loaded).

%% unregister_owner(Ctx, Pid): Pid owns nothing any more (its servers go back to the default owner of
%% start_collector/2) and its slot of the owner table is free for the next register_owner/4 -- call it from
%% ra_server_proc:terminate/3, so that restarts do not grow the table (src/ra_server_proc.erl terminate/3).
unregister_owner(_Ctx, _Pid) -> erlang:nif_error(not_loaded).

%% owner_slots(Ctx) -> {Slots, Live}: diagnostics of the owner table.
owner_slots(_Ctx) -> erlang:nif_error(not_loaded).

%% fan_back_stats(Ctx) -> {Batches, Decisions, Nanoseconds} spent by the collector thread fanning batches back.
fan_back_stats(_Ctx) -> erlang:nif_error(not_loaded).
%% submit/3 may be called from any process; batches above 2048 messages run on a dirty CPU scheduler.
submit(_Ctx, _MsgsBin, _Tick) -> erlang:nif_error(not_loaded).
%% submit/4: + the batch's range list, <<First:64/little, Last:64/little>> per entry -- the lower ranges of written
%% events whose ra_seq has more than two ranges (encode_msgs/2 builds both binaries)
submit(_Ctx, _MsgsBin, _Tick, _RangesBin) -> erlang:nif_error(not_loaded).
%% submit_raw/4: the batch travels as it is (one copy into the pinned slot); validation, the sub-tick rounds and the
%% bucket order run on the device.  MaxRounds = the caller's bound on the messages per server in the batch (1..8,
%% 0 = 4); a batch may hold at most the largest N with sum_{r < MaxRounds} N div (r + 1) =< RingCapacity messages.
%% Input errors are the BATCH's result: collect/1 returns {error, invalid | unsupported} once (the collector thread
%% sends {ra_gpu_batch_error, _} to the default owner), nothing of the batch is applied, the ring moves on.
%% A dirty IO-bound NIF at every size: the call waits for its turn behind the slots begun before it.
submit_raw(_Ctx, _MsgsBin, _Tick, _MaxRounds) -> erlang:nif_error(not_loaded).
collect(_Ctx) -> erlang:nif_error(not_loaded).
start_collector(_Ctx, _Pid) -> erlang:nif_error(not_loaded).
stop_collector(_Ctx) -> erlang:nif_error(not_loaded).
snapshot(_Ctx, _NGroups) -> erlang:nif_error(not_loaded).
%% The node-wide leaderboard over the GPUs of one node (one context per GPU, groups routed by route/2; the reference's
%% ra_leaderboard is one ETS table per node, src/ra_leaderboard.erl:18-26): RCCL all-gather behind the C ABI.
%% comm_unique_id() -> {ok, <<Id:128/binary>>} on ONE context's owner, Id sent to the others as a plain message;
%% comm_init(Ctx, Id, NRanks, Rank) -> ok and allgather_leaderboard(Ctx, NRows) -> {ok, RowsBin} are collective: the
%% owner process of every context calls them (dirty scheduler), NRows = the largest group count of any context.
comm_unique_id() -> erlang:nif_error(not_loaded).
comm_init(_Ctx, _Id, _NRanks, _Rank) -> erlang:nif_error(not_loaded).
allgather_leaderboard(_Ctx, _NRows) -> erlang:nif_error(not_loaded).

%% node_leaderboard(Ctx, NRows, GroupsOfRank) -> [{GroupUId, LeaderSlot | undefined, Term, CommitIndex, LastApplied}]
%% for EVERY group of the node, from this context's side of the collective: GroupsOfRank(Rank) -> [GroupUId] ascending
%% (the groups with route(GroupUId, NRanks) =:= Rank, in local-id order).  What ra_leaderboard:lookup_leader/1 and the
%% commit_index / last_applied gauges of ra:key_metrics/1 (src/ra.erl:1242-1270) read, for all GPUs at once.
node_leaderboard(Ctx, NRows, GroupsOfRank) ->
    {ok, Bin} = allgather_leaderboard(Ctx, NRows),
    RowBytes = 32,
    NRanks = byte_size(Bin) div (NRows * RowBytes),
    lists:append(
      [begin
           Shard = binary:part(Bin, Rank * NRows * RowBytes, NRows * RowBytes),
           [begin
                <<Leader:32/little, _NLeaders:32/little, Term:64/little, CI:64/little, LA:64/little>> =
                    binary:part(Shard, K * RowBytes, RowBytes),
                {UId, case Leader of 255 -> undefined; _ -> Leader end, Term, CI, LA}
            end || {K, UId} <- lists:zip(lists:seq(0, length(GroupsOfRank(Rank)) - 1), GroupsOfRank(Rank))]
       end || Rank <- lists:seq(0, NRanks - 1)]).
wal_checksums(_Ctx, _EntriesBin, _DataBin) -> erlang:nif_error(not_loaded).

wal_frame(_Ctx, _RecordsBin, _DataBin, _Flags) -> erlang:nif_error(not_loaded).
wal_recover_check(_Ctx, _FileBin) -> erlang:nif_error(not_loaded).

%% segments and snapshots: erlang:crc32/1,2 for a batch of entries, one long binary, a whole segment file
crc32s(_Ctx, _EntriesBin, _DataBin) -> erlang:nif_error(not_loaded).
crc32_stream(_Ctx, _Bin, _Init) -> erlang:nif_error(not_loaded).
segment_build(_Ctx, _EntriesBin, _DataBin, _MaxCount, _Flags) -> erlang:nif_error(not_loaded).

%% major compaction (src/ra_log_segments.erl:741-835): info/2 of the files of a compaction group, and the new
%% segment that holds their live entries.  SourcesBin = one 32-byte record per file, little endian:
%% offset:64, n_bytes:64 (the file inside FilesBin), live_first:32, live_n:32 (its {First, Last} pairs inside
%% LiveBin), 0:64; LiveBin = First:64/little, Last:64/little per pair, ascending and not adjacent per file.
%% InfosBin = one 64-byte record per file: size:64, index_size:64, live_size:64, range_first:64, range_last:64,
%% num_entries:32, num_indexes:32, max_count:32, version:32, status:32, 0:32.  LiveBin = <<>> for segment_info:
%% no live sequence (`undefined`).
segment_info(_Ctx, _SourcesBin, _FilesBin, _LiveBin) -> erlang:nif_error(not_loaded).
segment_compact(_Ctx, _SourcesBin, _FilesBin, _LiveBin, _MaxSize, _Flags) -> erlang:nif_error(not_loaded).

%% Group = [{FileBin, LiveSeq}], oldest file first, LiveSeq the ra_seq:state() of the indexes to keep from that file
%% (ra_seq:in_range/2 and the progressive ra_seq:limit/2 of src/ra_log_segments.erl:745-761 are the caller's).
%% -> {ok, SegmentBin}, the bytes ra_log_segment:copy/3 would have left in the new file after the last source
%% (src/ra_log_segment.erl:819-908), or what copy/3 / append_raw/6 would have failed with:
%% {error, {copy_missing_key, Idx}} | {error, full} | {error, {truncated | space | crc, SourceNo, Idx}}.
%% Opening, writing and renaming files, symlinks and compaction markers stay in ra_log_segments.
segment_compact_group(Ctx, Group, MaxSize, Verify) ->
    {SourcesBin, Files, LiveBin, _, _} =
        lists:foldl(fun({FileBin, LiveSeq}, {S, F, L, Off, LiveOff}) ->
                            Ranges = seq_ranges(LiveSeq),
                            Len = byte_size(FileBin),
                            N = length(Ranges),
                            {<<S/binary, Off:64/little, Len:64/little, LiveOff:32/little, N:32/little, 0:64>>,
                             [F, FileBin],
                             << L/binary, << <<Lo:64/little, Hi:64/little>> || {Lo, Hi} <- Ranges >>/binary >>,
                             Off + Len, LiveOff + N}
                    end, {<<>>, [], <<>>, 0, 0}, Group),
    Flags = case Verify of true -> 1; false -> 0 end,
    segment_compact(Ctx, SourcesBin, iolist_to_binary(Files), LiveBin, MaxSize, Flags).

%% major compaction for many members in one call: the plan, then the copy of every group (the .compaction_group
%% marker of src/ra_log_segments.erl:783-786 is written between the two).  MembersBin = one 16-byte record per member:
%% segref_first:32, segref_n:32 (its files inside SegrefsBin, newest first as compactable_segrefs/2 gives them),
%% live_first:32, live_n:32 (its live pairs inside LiveBin).  SegrefsBin = one 32-byte record per file: offset:64,
%% n_bytes:64 (the file inside FilesBin), range_first:64, range_last:64.  RowsBin = one 32-byte record per file:
%% num_live:64, live_first:32, live_n:32 (its selection inside LiveOutBin), flags:32 (1 = unreferenced: the Delete list
%% of both compaction kinds), group:32 (its group in GroupsBin, 16#FFFFFFFF = none), status:32 (1 = the member's
%% take_group/3 would have raised badarith), 0:32.  GroupsBin = one 24-byte record per group: src_first:32, src_n:32,
%% out_offset:64, out_bytes:64; the sources of the copy are the groups' files in GroupsBin order, oldest first.
%% ResultsBin = one 32-byte record per group: status:32, n_entries:32, file_bytes:64, index:64, source:32, 0:32.
%% A file with live indexes whose header is damaged makes segment_compact_plan answer {error, invalid} for the whole
%% call (info/2 would crash that member's compaction); segment_compact_groups fails only that file's group.
segment_compact_plan(_Ctx, _MembersBin, _SegrefsBin, _FilesBin, _LiveBin, _MaxCount, _MaxSize) ->
    erlang:nif_error(not_loaded).
segment_compact_groups(_Ctx, _GroupsBin, _SourcesBin, _FilesBin, _LiveBin, _MaxSize, _Flags) ->
    erlang:nif_error(not_loaded).

%% Members = [{[{FileBin, Range}], LiveSeq}]: per member its compactable files newest first with their segref ranges
%% and its live indexes; Conf = #{max_count := _, max_size := _} (the compaction conf, also the segments' max_size).
%% -> [{Unreferenced, [{GroupFileOrdinals, {ok, SegmentBin} | {error, _}}]}] per member: the ordinals (from 0) of the
%% files without live indexes, and per group the ordinals of its files oldest first (the head is the group leader) with
%% the new segment or what segment_compact_group/4 would have failed with.  A member whose grouping would have
%% raised badarith has no groups.  Markers, renames, symlinks, deletes and sync_dir stay in ra_log_segments.
major_compaction_batch(Ctx, Members, #{max_count := MaxCount, max_size := MaxSize}, Verify) ->
    {MembersBin, SegrefsBin, Files, LiveBin, _, _, _} =
        lists:foldl(
          fun({FileRanges, LiveSeq}, {M, S, F, L, RefOff, FileOff, LiveOff}) ->
                  Ranges = seq_ranges(LiveSeq),
                  {S1, F1, FileOff1} =
                      lists:foldl(fun({FileBin, {First, Last}}, {S0, F0, Off}) ->
                                          Len = byte_size(FileBin),
                                          {<<S0/binary, Off:64/little, Len:64/little, First:64/little, Last:64/little>>,
                                           [F0, FileBin], Off + Len}
                                  end, {S, F, FileOff}, FileRanges),
                  NRefs = length(FileRanges),
                  NLive = length(Ranges),
                  {<<M/binary, RefOff:32/little, NRefs:32/little, LiveOff:32/little, NLive:32/little>>, S1, F1,
                   << L/binary, << <<Lo:64/little, Hi:64/little>> || {Lo, Hi} <- Ranges >>/binary >>,
                   RefOff + NRefs, FileOff1, LiveOff + NLive}
          end, {<<>>, <<>>, [], <<>>, 0, 0, 0}, Members),
    FilesBin = iolist_to_binary(Files),
    {ok, RowsBin, GroupsBin, LiveOutBin} =
        segment_compact_plan(Ctx, MembersBin, SegrefsBin, FilesBin, LiveBin, MaxCount, MaxSize),
    Rows = [{LiveFirst, LiveN, Flags, Group}
            || <<_NumLive:64/little, LiveFirst:32/little, LiveN:32/little, Flags:32/little, Group:32/little,
                 _Status:32/little, _:32>> <= RowsBin],
    Refs = [{Off, Len} || <<Off:64/little, Len:64/little, _:128>> <= SegrefsBin],
    %% the sources of the copy: group by group, a group's files oldest first = its rows last to first
    Tagged = lists:zip3(lists:seq(0, length(Rows) - 1), Rows, Refs),
    %% (lists:sort/1 on the whole tuple: by group, then by -K, i.e. the member's LAST segref first)
    InGroups = lists:sort([{Group, -K, Off, Len, LiveFirst, LiveN}
                           || {K, {LiveFirst, LiveN, _, Group}, {Off, Len}} <- Tagged, Group =/= 16#FFFFFFFF]),
    SourcesBin = << <<Off:64/little, Len:64/little, LiveFirst:32/little, LiveN:32/little, 0:64>>
                    || {_, _, Off, Len, LiveFirst, LiveN} <- InGroups >>,
    Flags = case Verify of true -> 1; false -> 0 end,
    {ok, ResultsBin, OutBin} =
        segment_compact_groups(Ctx, GroupsBin, SourcesBin, FilesBin, LiveOutBin, MaxSize, Flags),
    Groups = [{OutOff, OutLen} || <<_:64, OutOff:64/little, OutLen:64/little>> <= GroupsBin],
    Results = [R || <<R:32/binary>> <= ResultsBin],
    Answers = [compact_groups_answer(R, OutOff, OutBin) || {R, {OutOff, _}} <- lists:zip(Results, Groups)],
    {PerMember, _} =
        lists:mapfoldl(
          fun({FileRanges, _}, RefOff) ->
                  N = length(FileRanges),
                  Mine = [{K - RefOff, Row} || {K, Row, _} <- Tagged, K >= RefOff, K < RefOff + N],
                  Unref = [K || {K, {_, _, F, _}} <- Mine, F band 1 =:= 1],
                  Gs = lists:usort([G || {_, {_, _, _, G}} <- Mine, G =/= 16#FFFFFFFF]),
                  {{Unref, [{lists:reverse([K || {K, {_, _, _, G1}} <- Mine, G1 =:= G]), lists:nth(G + 1, Answers)}
                            || G <- Gs]}, RefOff + N}
          end, 0, Members),
    PerMember.

compact_groups_answer(<<0:32/little, _:32, FileBytes:64/little, _/binary>>, OutOff, OutBin) ->
    {ok, binary:part(OutBin, OutOff, FileBytes)};
compact_groups_answer(<<1:32/little, _:32, _:64, Idx:64/little, _/binary>>, _, _) -> {error, {copy_missing_key, Idx}};
compact_groups_answer(<<2:32/little, _/binary>>, _, _) -> {error, full};
compact_groups_answer(<<St:32/little, _:32, _:64, Idx:64/little, Source:32/little, _:32>>, _, _) ->
    {error, {case St of 3 -> truncated; 4 -> space; 5 -> crc; 6 -> bad_source end, Source, Idx}}.

%% mem-table flush (src/ra_log_segment_writer.erl:268-329, 425-500): the entries of every writer of a rolled-over WAL
%% appended to the writers' segment files in one call.  WritersBin = one 48-byte record per writer, little endian:
%% entry_first:32, entry_n:32 (its entries inside EntriesBin), open_count:32, open_max_count:32, open_data_bytes:64,
%% range_first:64, range_last:64 (16#FFFFFFFFFFFFFFFF twice for `undefined`), 0:64.  EntriesBin as for crc32s.
%% PiecesBin = one 80-byte record per run of entries in one file, sorted by writer and file: writer:32, ordinal:32,
%% entry_first:32, entry_n:32, index_file_off:64, data_file_off:64, out_index_off:64, out_data_off:64, data_bytes:64,
%% range_first:64, range_last:64, max_count:32, 0:32.
segment_flush(_Ctx, _WritersBin, _EntriesBin, _DataBin, _MaxCount, _MaxSize, _Flags) -> erlang:nif_error(not_loaded).

%% Writers = [{OpenState, [{Idx, Term, Bin}]}], OpenState = {Count, MaxCount, DataBytes, Range} of the writer's open
%% segment (Count = (index_offset - 8) div 32, DataBytes = data_offset - data_start, Range = ra_log_segment:range/1:
%% `undefined` or {First, Last}), the entries in append order.  -> {ok, PerWriter}: per writer, in file order,
%% [{Ordinal, IndexFileOff, IndexIoData, DataFileOff, DataBin, Range}]: Ordinal 0 is the open segment, K its K-th
%% successor (zpad_filename_incr K times, opened with MaxCount); IndexIoData goes to IndexFileOff -- for a successor
%% it starts with the file header, at offset 0 -- and DataBin to DataFileOff; Range is the file's range afterwards.
%% Opening and naming files, file:pwrite, sync, the ra_seq selection of what to flush and the `segments` notification
%% stay in ra_log_segment_writer; an open segment of version 1 is finished through ra_log_segment itself.
segment_flush_batch(Ctx, Writers, MaxCount, MaxSize, ComputeChecksums) ->
    Undef = 16#FFFFFFFFFFFFFFFF,
    {WritersBin, EntriesBin, Data, _, _} =
        lists:foldl(fun({{Count, OpenMax, DataBytes, Range}, Entries}, {W, E0, D0, First, Off0}) ->
                            {RF, RL} = case Range of undefined -> {Undef, Undef}; _ -> Range end,
                            {E1, D1, Off1} =
                                lists:foldl(fun({Idx, Term, Bin}, {E, D, Off}) ->
                                                    Len = byte_size(Bin),
                                                    {<<E/binary, Idx:64/little, Term:64/little, Off:64/little,
                                                       Len:32/little, 0:32>>, [D, Bin], Off + Len}
                                            end, {E0, D0, Off0}, Entries),
                            N = length(Entries),
                            {<<W/binary, First:32/little, N:32/little, Count:32/little, OpenMax:32/little,
                               DataBytes:64/little, RF:64/little, RL:64/little, 0:64>>, E1, D1, First + N, Off1}
                    end, {<<>>, <<>>, [], 0, 0}, Writers),
    Flags = case ComputeChecksums of true -> 0; false -> 1 end,
    case segment_flush(Ctx, WritersBin, EntriesBin, iolist_to_binary(Data), MaxCount, MaxSize, Flags) of
        {ok, PiecesBin, Out} ->
            Pieces = [{W, Ord, N, IFO, DFO, OIO, ODO, DB, {RF, RL}} ||
                         <<W:32/little, Ord:32/little, _EF:32/little, N:32/little, IFO:64/little, DFO:64/little,
                           OIO:64/little, ODO:64/little, DB:64/little, RF:64/little, RL:64/little, _MC:32/little,
                           _:32>> <= PiecesBin],
            Out1 = fun({_W, 0, N, IFO, DFO, OIO, ODO, DB, R}) ->
                           {0, IFO, binary:part(Out, OIO, 32 * N), DFO, binary:part(Out, ODO, DB), R};
                      ({_W, Ord, N, _IFO, DFO, OIO, ODO, DB, R}) ->
                           {Ord, 0, binary:part(Out, OIO - 8, 8 + 32 * N), DFO, binary:part(Out, ODO, DB), R}
                   end,
            {ok, flush_pieces_by_writer(Pieces, 0, length(Writers), Out1)};
        Error ->
            Error
    end.

%% the pieces are sorted by writer: one pass
flush_pieces_by_writer(_Pieces, WNo, NWriters, _Out1) when WNo >= NWriters -> [];
flush_pieces_by_writer(Pieces, WNo, NWriters, Out1) ->
    {Mine, Rest} = lists:splitwith(fun(P) -> element(1, P) =:= WNo end, Pieces),
    [[Out1(P) || P <- Mine] | flush_pieces_by_writer(Rest, WNo + 1, NWriters, Out1)].

%% reading entries back (src/ra_log_segment.erl:340-359, 375-598, 652-689; src/ra_log_segments.erl:398-622): the read
%% plans of any number of segment files, of any number of servers, in one call.  SourcesBin = one 32-byte record per
%% file, little endian: offset:64, n_bytes:64 (the file inside FilesBin), req_first:32, req_n:32 (its indexes inside
%% ReqBin), 0:64; ReqBin = Idx:64/little per requested index, in the caller's order.  RowsBin = one 32-byte record per
%% request: idx:64, term:64, data_offset:64 (into OutBin; with Flags 2 into FilesBin; 16#FFFFFFFFFFFFFFFF: no such
%% entry), data_len:32, crc:32.  ResultsBin = one 32-byte record per file: status:32 (0 ok, 1 missing, 2 truncated,
%% 3 crc, 4 bad segment), n_read:32, index:64, data_bytes:64, 0:64.  Flags: 1 = validate checksums, 2 = rows only.
segment_read(_Ctx, _SourcesBin, _FilesBin, _ReqBin, _Flags) -> erlang:nif_error(not_loaded).

%% the descriptors of Plan = [{FileBin, [Idx]}]
read_plan_bins(Plan) ->
    {SourcesBin, Files, ReqBin, _, _} =
        lists:foldl(fun({FileBin, Idxs}, {S, F, Q, Off, First}) ->
                            Len = byte_size(FileBin),
                            N = length(Idxs),
                            {<<S/binary, Off:64/little, Len:64/little, First:32/little, N:32/little, 0:64>>,
                             [F, FileBin],
                             << Q/binary, << <<I:64/little>> || I <- Idxs >>/binary >>,
                             Off + Len, First + N}
                    end, {<<>>, [], <<>>, 0, 0}, Plan),
    {SourcesBin, iolist_to_binary(Files), ReqBin}.

%% Plan = [{FileBin, [Idx]}]: per segment file the indexes to read, in any order (read_sparse/4; a fold of From..To is
%% lists:seq(From, To)).  Opts: validate => boolean() (fold0's validate_checksum, default false), strategy => error |
%% return (what a fold does with a missing key, default error).  -> {ok, [Answer]}, one per file, in order:
%% {ok, [{Idx, Term, Bin}]} | {error, {missing_key, Idx}} | {error, {read_error, Idx}} |
%% {error, {crc_check_failure, Idx}} | {error, bad_segment}; with strategy => return a missing key gives
%% {ok, Prefix}, the entries in front of it.  One file's error leaves the other files' answers as they are.
%% The ra_lol search of the segrefs, is_modified/1, the fd LRU, binary_to_term, the mem-table overlay and file I/O
%% stay in ra_log_segments.
segment_read_plan(Ctx, Plan, Opts) ->
    Flags = case maps:get(validate, Opts, false) of true -> 1; false -> 0 end,
    Strategy = maps:get(strategy, Opts, error),
    {SourcesBin, FilesBin, ReqBin} = read_plan_bins(Plan),
    case segment_read(Ctx, SourcesBin, FilesBin, ReqBin, Flags) of
        {ok, RowsBin, ResultsBin, Out} ->
            Entries = fun(Rows) ->
                              [{Idx, Term, binary:part(Out, Off, Len)} ||
                                  <<Idx:64/little, Term:64/little, Off:64/little, Len:32/little, _Crc:32>> <= Rows]
                      end,
            {ok, read_plan_answers(Plan, ResultsBin, RowsBin, 0,
                                   fun(0, _NRead, _Idx, Rows) -> {ok, Entries(Rows)};
                                      (1, NRead, _Idx, Rows) when Strategy =:= return ->
                                           {ok, Entries(binary:part(Rows, 0, 32 * NRead))};
                                      (1, _NRead, Idx, _Rows) -> {error, {missing_key, Idx}};
                                      (2, _NRead, Idx, _Rows) -> {error, {read_error, Idx}};
                                      (3, _NRead, Idx, _Rows) -> {error, {crc_check_failure, Idx}};
                                      (4, _NRead, _Idx, _Rows) -> {error, bad_segment}
                                   end)};
        Error ->
            Error
    end.

%% Plan as for segment_read_plan/3 -> {ok, [Answer]}, one per file: {ok, [Term | undefined]} in the order of the
%% file's indexes (term_query/2) | {error, bad_segment}.  No payload is touched.  One difference from term_query/2:
%% an index whose record points outside its file (a truncated file) answers `undefined` here, the Term there.
segment_term_query_batch(Ctx, Plan) ->
    Undef = 16#FFFFFFFFFFFFFFFF,
    {SourcesBin, FilesBin, ReqBin} = read_plan_bins(Plan),
    case segment_read(Ctx, SourcesBin, FilesBin, ReqBin, 2) of
        {ok, RowsBin, ResultsBin, _Out} ->
            {ok, read_plan_answers(Plan, ResultsBin, RowsBin, 0,
                                   fun(4, _NRead, _Idx, _Rows) -> {error, bad_segment};
                                      (_St, _NRead, _Idx, Rows) ->
                                           {ok, [case Off of Undef -> undefined; _ -> Term end ||
                                                    <<_Idx:64/little, Term:64/little, Off:64/little, _:64>> <= Rows]}
                                   end)};
        Error ->
            Error
    end.

%% the files' slices of RowsBin follow each other in plan order: one pass
read_plan_answers([], <<>>, _RowsBin, _First, _Answer) -> [];
read_plan_answers([{_FileBin, Idxs} | Plan], <<St:32/little, NRead:32/little, Idx:64/little, _:128, Results/binary>>,
                  RowsBin, First, Answer) ->
    N = length(Idxs),
    [Answer(St, NRead, Idx, binary:part(RowsBin, 32 * First, 32 * N)) |
     read_plan_answers(Plan, Results, RowsBin, First + N, Answer)].

%% snapshots and checkpoints (src/ra_log_snapshot.erl, src/ra_snapshot.erl:343-479, 1008-1059): ragged CRC batches, the
%% snapshot.dat / indexes images and their validation, for many members in one call.  All records little endian.
%% SpansBin = one 32-byte record per span: offset:64, n_bytes:64 (inside DataBin), init:32, 0:96; CrcsBin = Crc:32 each.
%% ItemsBin = one 40-byte record per image: kind:32 (0 snapshot, 1 indexes), meta_len:32, meta_offset:64,
%% data_offset:64, data_bytes:64 (inside DataBin), out_offset:64 (filled by the NIF); ImagesBin = the images back to back.
%% FilesBin = one 32-byte record per file: offset:64, n_bytes:64 (inside BytesBin), kind:32, flags:32 (1 = the header
%% alone, read_meta/1), 0:64; InfosBin = one 48-byte record per file: status:32 (0 ok, 1 invalid_format,
%% 2 invalid_version, 3 checksum_error, 4 bad meta, 5 eof), version:32, stored_crc:32, computed_crc:32, meta_offset:64,
%% meta_len:32, 0:32, data_offset:64, data_bytes:64 (offsets into BytesBin).
crc32_spans(_Ctx, _SpansBin, _DataBin) -> erlang:nif_error(not_loaded).
snapshot_build(_Ctx, _ItemsBin, _DataBin) -> erlang:nif_error(not_loaded).
snapshot_validate(_Ctx, _FilesBin, _BytesBin) -> erlang:nif_error(not_loaded).

%% Snapshots = [{MetaBin, DataIoList}] (MetaBin = term_to_binary(Meta), DataIoList = term_to_iovec(MacState)) ->
%% {ok, [ImageBin]}: what ra_log_snapshot:write/4 hands to ra_lib:write_file/3 (:49-68), for every member that writes a
%% snapshot or checkpoint after a WAL roll-over.  term_to_binary / term_to_iovec, file I/O and fsync stay with the caller.
snapshot_images(Ctx, Snapshots) ->
    {ItemsBin, Data, _, Sizes} =
        lists:foldl(fun({MetaBin, DataIoList}, {I, D, Off, S}) ->
                            MLen = byte_size(MetaBin),
                            DLen = iolist_size(DataIoList),
                            {<<I/binary, 0:32/little, MLen:32/little, Off:64/little, (Off + MLen):64/little,
                               DLen:64/little, 0:64>>,
                             [D, MetaBin, DataIoList], Off + MLen + DLen, [13 + MLen + DLen | S]}
                    end, {<<>>, [], 0, []}, Snapshots),
    case snapshot_build(Ctx, ItemsBin, iolist_to_binary(Data)) of
        {ok, ImagesBin} -> {ok, split_images(ImagesBin, lists:reverse(Sizes))};
        Error -> Error
    end.

split_images(<<>>, []) -> [];
split_images(Bin, [Size | Sizes]) ->
    <<Image:Size/binary, Rest/binary>> = Bin,
    [Image | split_images(Rest, Sizes)].

%% Files = [{FileBin, validate | read_meta}], the snapshot.dat bytes of a recovery batch -- per member its snapshot
%% (validate), its newest checkpoint (validate), older checkpoints (read_meta): pick_first_valid/4, find_checkpoints/4,
%% find_recovery_checkpoint/1 (src/ra_snapshot.erl:343-479).  -> {ok, [Answer]}, one per file, in order:
%% {ok, MetaBin, DataBin} (for binary_to_term) | {error, invalid_format} | {error, {invalid_version, V}} |
%% {error, checksum_error} | {error, bad_meta} (parse_snapshot/1 has no clause; read_meta: the short read) |
%% {error, unexpected_eof_when_parsing_header}.  One file's error leaves the other files' answers as they are.
%% Directory listing and sorting, which file to try next and what to delete stay in ra_snapshot.
snapshot_recover_batch(Ctx, Files) ->
    {FilesBin, Bytes, _} =
        lists:foldl(fun({FileBin, Mode}, {F, B, Off}) ->
                            Len = byte_size(FileBin),
                            Flags = case Mode of validate -> 0; read_meta -> 1 end,
                            {<<F/binary, Off:64/little, Len:64/little, 0:32/little, Flags:32/little, 0:64>>,
                             [B, FileBin], Off + Len}
                    end, {<<>>, [], 0}, Files),
    BytesBin = iolist_to_binary(Bytes),
    case snapshot_validate(Ctx, FilesBin, BytesBin) of
        {ok, InfosBin} ->
            {ok, [case St of
                      0 -> {ok, binary:part(BytesBin, MOff, MLen), binary:part(BytesBin, DOff, DLen)};
                      1 -> {error, invalid_format};
                      2 -> {error, {invalid_version, V}};
                      3 -> {error, checksum_error};
                      4 -> {error, bad_meta};
                      5 -> {error, unexpected_eof_when_parsing_header}
                  end ||
                     <<St:32/little, V:32/little, _Stored:32, _Computed:32, MOff:64/little, MLen:32/little, _:32,
                       DOff:64/little, DLen:64/little>> <= InfosBin]};
        Error ->
            Error
    end.

%% Chunks = [{PartialCrc0, ChunkBin}], one per snapshot transfer in flight -> [PartialCrc]:
%% erlang:crc32(PartialCrc0, Chunk) of accept_chunk/2 (src/ra_log_snapshot.erl:104-108); PartialCrc0 = 0 starts a
%% checksum (begin_accept/2, :80-81).  The file:write of the chunk and the pwrite of the Crc at byte 5 in
%% complete_accept/2 stay with the caller.
accept_chunks(Ctx, Chunks) ->
    {SpansBin, Data, _} =
        lists:foldl(fun({Crc0, ChunkBin}, {S, D, Off}) ->
                            Len = byte_size(ChunkBin),
                            {<<S/binary, Off:64/little, Len:64/little, Crc0:32/little, 0:96>>, [D, ChunkBin], Off + Len}
                    end, {<<>>, [], 0}, Chunks),
    {ok, CrcsBin} = crc32_spans(Ctx, SpansBin, iolist_to_binary(Data)),
    [Crc || <<Crc:32/little>> <= CrcsBin].

%% The bytes of a whole segment file for Entries = [{Idx, Term, Bin}] in the caller's order: what
%% ra_log_segment:append/4 accumulates in pending_index / pending_data and flush/1 writes
%% (src/ra_log_segment.erl:262-338); is_full/1 and the file I/O stay with the caller.
segment_image(Ctx, Entries, MaxCount, ComputeChecksums) ->
    {EntriesBin, Data, _} =
        lists:foldl(fun({Idx, Term, Bin}, {E, D, Off}) ->
                            Len = byte_size(Bin),
                            {<<E/binary, Idx:64/little, Term:64/little, Off:64/little,
                               Len:32/little, 0:32>>, [D, Bin], Off + Len}
                    end, {<<>>, [], 0}, Entries),
    Flags = case ComputeChecksums of true -> 0; false -> 1 end,
    {ok, Image} = segment_build(Ctx, EntriesBin, iolist_to_binary(Data), MaxCount, Flags),
    Image.

%% ra_log_wal:write_data/8 computes erlang:adler32([<<Idx:64, Term:64>> | EntryData]) per record
%% (src/ra_log_wal.erl:528-534); for a whole write_batch: Entries = [{Idx, Term, Bin}].
wal_batch_checksums(Ctx, Entries) ->
    {EntriesBin, Data, _} =
        lists:foldl(fun({Idx, Term, Bin}, {E, D, Off}) ->
                            Len = byte_size(Bin),
                            {<<E/binary, Idx:64/little, Term:64/little, Off:64/little,
                               Len:32/little, 0:32>>, [D, Bin], Off + Len}
                    end, {<<>>, [], 0}, Entries),
    {ok, Sums} = wal_checksums(Ctx, EntriesBin, iolist_to_binary(Data)),
    [C || <<C:32/little>> <= Sums].

%% The record bytes of a whole WAL batch.  Records = [{HeaderData, Idx, Term, EntryData}] where
%% HeaderData is what ra_log_wal:serialize_header/3 returned for the writer (the writer-name cache
%% stays in #wal{}); the result is the iodata write_data/8 would have accumulated in
%% #batch.pending (src/ra_log_wal.erl:513-537), ready for file:write/2 in flush_pending/1.
wal_frame_batch(Ctx, Records, ComputeChecksums) ->
    {RecsBin, Data, _} =
        lists:foldl(fun({Hdr, Idx, Term, Bin}, {R, D, Off}) ->
                            HLen = byte_size(Hdr),
                            Len = byte_size(Bin),
                            {<<R/binary, Idx:64/little, Term:64/little, (Off + HLen):64/little,
                               Len:32/little, HLen:32/little, Off:64/little, 0:64>>,
                             [D, Hdr, Bin], Off + HLen + Len}
                    end, {<<>>, [], 0}, Records),
    Flags = case ComputeChecksums of true -> 0; false -> 1 end,
    {ok, Framed} = wal_frame(Ctx, RecsBin, iolist_to_binary(Data), Flags),
    Framed.

%% WAL batch (src/ra_log_wal.erl:482-635, 800-812, 1050-1066): handle_batch/2 for a mailbox-ordered run of append
%% commands in one call.  All records little endian.  CmdsBin = 64 bytes per command: writer:32 (slot in WritersBin),
%% data_len:32, index:64, term:64, prev_index:64, smallest_index:64, tid:64, data_offset:64, 0:64.  WritersBin = 32
%% bytes per slot: state:32 (0 undefined, 1 in_seq, 2 out_of_seq), id_ref:32 (16#FFFFFFFF: not in this file's
%% writer-name cache), prev_index:64, uid_offset:64, uid_len:32, 0:32.  FileBin = file_size:64, entry_count:64,
%% max_size:64, max_entries:64 (0 = undefined), next_id_ref:32, 0:32.  ResultsBin = 16 bytes per command:
%% verdict:32 (low byte 0 not consumed, 1 write, 2 drop, 3 ignore, 4 resend; 16#100 Trunc, 16#200 long header),
%% checksum:32, value:64 (write: offset in FramedBin; resend: the index to resend from).  EventsBin = 32 bytes per
%% event: writer:32, range_first:32, term:64, tid:64, range_n:32, 0:32; RangesBin = first:64, last:64 per pair.
%% TotalBin = status:32 (0 ok, 1 roll), n_consumed:32, n_written:32, n_events:32, n_ranges:32, next_id_ref:32,
%% out_bytes:64, file_size:64, entry_count:64, 0:128.
wal_batch(_Ctx, _CmdsBin, _WritersBin, _FileBin, _DataBin, _Flags) -> erlang:nif_error(not_loaded).

%% Cmds = [{Slot, MtTid, ExpectedPrevIdx, Idx, Term, SmallestIdx, EntryBin}] in mailbox order, MtTid an integer the
%% caller maps its ets tids to, ExpectedPrevIdx -1 passed as 0 (both compare the same with every P >= 0);
%% Writers = [{State, IdRef, UId}] by slot, State = undefined | {in_seq, P} | {out_of_seq, P}, IdRef = the 22-bit
%% number of the writer-name cache or undefined; File = {FileSize, EntryCount, MaxSize, MaxEntries | undefined, NextIdRef}.
%% -> {Verdicts, FramedBin, Writers1, [{Slot, Term, MtTid, Seq}], File1, ok | {roll, NConsumed}}: Verdicts = one of
%% write | drop | ignore | {resend, Idx} | not_consumed per command; FramedBin goes to file:write/2 as
%% flush_pending/1's Pend; every {Slot, Term, MtTid, Seq} is a `written` event (Seq a ra_seq built from the pairs) and
%% the input of update_ranges/5.  With {roll, N} the caller completes the batch, rolls the file and calls again with
%% lists:nthtail(N, Cmds), Writers1 with every IdRef undefined, and the new file.  rollover, forget_writer and query
%% messages, a UId whose Pid changes, counters, file I/O and sync stay in ra_log_wal.
wal_handle_batch(Ctx, Cmds, Writers, {FileSize, EntryCount, MaxSize, MaxEntries0, NextIdRef}, ComputeChecksums) ->
    MaxEntries = case MaxEntries0 of undefined -> 0; _ -> MaxEntries0 end,
    {WritersBin, UIds, Off0} =
        lists:foldl(fun({State, IdRef0, UId}, {W, D, Off}) ->
                            {Kind, P} = case State of
                                            undefined -> {0, 0};
                                            {in_seq, P0} -> {1, P0};
                                            {out_of_seq, P0} -> {2, P0}
                                        end,
                            IdRef = case IdRef0 of undefined -> 16#FFFFFFFF; _ -> IdRef0 end,
                            Len = byte_size(UId),
                            {<<W/binary, Kind:32/little, IdRef:32/little, P:64/little, Off:64/little, Len:32/little,
                               0:32>>, [D, UId], Off + Len}
                    end, {<<>>, [], 0}, Writers),
    {CmdsBin, Data, _} =
        lists:foldl(fun({Slot, Tid, Prev0, Idx, Term, Smallest, Bin}, {C, D, Off}) ->
                            Len = byte_size(Bin),
                            Prev = max(Prev0, 0),
                            {<<C/binary, Slot:32/little, Len:32/little, Idx:64/little, Term:64/little, Prev:64/little,
                               Smallest:64/little, Tid:64/little, Off:64/little, 0:64>>, [D, Bin], Off + Len}
                    end, {<<>>, UIds, Off0}, Cmds),
    FileBin = <<FileSize:64/little, EntryCount:64/little, MaxSize:64/little, MaxEntries:64/little,
                NextIdRef:32/little, 0:32>>,
    Flags = case ComputeChecksums of true -> 0; false -> 1 end,
    {ok, {ResultsBin, WritersBin1}, Framed, {EventsBin, RangesBin}, TotalBin} =
        wal_batch(Ctx, CmdsBin, WritersBin, FileBin, iolist_to_binary(Data), Flags),
    <<Status:32/little, NConsumed:32/little, _NWritten:32/little, _NEvents:32/little, _NRanges:32/little,
      NextIdRef1:32/little, _OutBytes:64/little, FileSize1:64/little, EntryCount1:64/little, _:128>> = TotalBin,
    Verdicts = [case V band 16#FF of
                    0 -> not_consumed; 1 -> write; 2 -> drop; 3 -> ignore; 4 -> {resend, Value}
                end || <<V:32/little, _Sum:32, Value:64/little>> <= ResultsBin],
    Writers1 = lists:zipwith(fun(<<Kind:32/little, IdRef:32/little, P:64/little, _:128>>, {_, _, UId}) ->
                                     {case Kind of 0 -> undefined; 1 -> {in_seq, P}; 2 -> {out_of_seq, P} end,
                                      case IdRef of 16#FFFFFFFF -> undefined; _ -> IdRef end, UId}
                             end, [W || <<W:32/binary>> <= WritersBin1], Writers),
    Pairs = list_to_tuple([{F, L} || <<F:64/little, L:64/little>> <= RangesBin]),
    Events = [{Slot, Term, Tid,
               lists:foldl(fun(K, Seq) ->
                                   case element(K, Pairs) of
                                       {I, I} -> [I | Seq];
                                       {F, L} when L =:= F + 1 -> [L, F | Seq];
                                       Range -> [Range | Seq]
                                   end
                           end, [], lists:seq(RF + 1, RF + RN))}
              || <<Slot:32/little, RF:32/little, Term:64/little, Tid:64/little, RN:32/little, _:32>> <= EventsBin],
    {Verdicts, Framed, Writers1, Events, {FileSize1, EntryCount1, MaxSize, MaxEntries0, NextIdRef1},
     case Status of 0 -> ok; 1 -> {roll, NConsumed} end}.

%% Recovery of one WAL file (src/ra_log_wal.erl:877-1033): the walk and every checksum in one
%% call; returns the records to hand to recover_entry/5, in file order, or throws like the
%% reference.  IsRegistered = fun(UId) -> boolean() (ra_directory:is_registered_uid/2).
wal_recover(Ctx, FileBin) ->
    {ok, Scanned, NOk, Status} = wal_recover_check(Ctx, FileBin),
    Status =:= corrupt andalso throw(wal_checksum_validation_failure),
    Recs = [R || <<R:56/binary>> <= Scanned],
    {Good, _} = lists:split(NOk, Recs),
    {_, Out} =
        lists:foldl(
          fun(<<Idx:64/little, Term:64/little, DOff:64/little, DLen:32/little, _Crc:32/little,
                UOff:64/little, IdRef:32/little, ULen:16/little, Trunc:8, Flags:8, _Next:64/little>>,
              {Names0, Acc}) ->
                  Names = case Flags band 1 of
                              1 -> Names0#{IdRef => binary:part(FileBin, UOff, ULen)};
                              0 -> Names0
                          end,
                  case Flags band 4 of
                      4 -> {Names, Acc};            %% IdRef of a deleted writer: skipped
                      0 -> {Names, [{maps:get(IdRef, Names), Trunc =:= 1, Idx, Term,
                                     binary:part(FileBin, DOff, DLen)} | Acc]}
                  end
          end, {#{}, []}, Good),
    lists:reverse(Out).

%% encode_msgs([{Server, Msg, Slot}]) -> {MsgsBin, RangesBin} | {fallback, Server}: a whole batch for submit/4 -- the
%% records in order, and the range list that written events of more than two ranges refer to (empty for most batches:
%% submit/3 will do).
encode_msgs(Items) ->
    encode_msgs(Items, <<>>, <<>>).
encode_msgs([], Msgs, Ranges) -> {Msgs, Ranges};
encode_msgs([{Server, Msg, Slot} | Rest], Msgs, Ranges) ->
    case encode_msg(Server, Msg, Slot) of
        fallback -> {fallback, Server};
        {seqx, Record, Lower} ->
            encode_msgs(Rest, <<Msgs/binary, (Record(byte_size(Ranges) div 16))/binary>>, <<Ranges/binary, Lower/binary>>);
        Bin when is_binary(Bin) -> encode_msgs(Rest, <<Msgs/binary, Bin/binary>>, Ranges)
    end.

%% Slot = fun(ra_server_id()) -> 0..7 | 255, the member slot of a server id inside its group.
%% Returns the 64-byte record, or `fallback` for an event the batched path does not take (the caller runs
%% ra_server:handle_* itself and re-uploads the server's integers with upload_state/3).  Every message kind
%% of include/ra_gpu_batch.h has a clause; anything else (install_snapshot, cluster changes, ..) is not a
%% message of this path and must not be passed in.
encode_msg(Server, #append_entries_rpc{term = T, leader_id = L, leader_commit = LC,
                                       prev_log_index = PI, prev_log_term = PT,
                                       entries = Entries}, Slot) ->
    %% entries are contiguous; at most two term runs ride inline (payloads stay on the host)
    {N, N0, T0, T1, Gap} = entry_runs(PI, Entries),
    <<Server:32/little, ?MSG_AER:8, (Slot(L)):8, 0:8, Gap:8, T:64/little, PI:64/little,
      PT:64/little, LC:64/little, N:32/little, N0:32/little, T0:64/little, T1:64/little>>;
encode_msg(Server, {Peer, #append_entries_reply{term = T, success = S, next_index = NI,
                                                 last_index = LI, last_term = LT}}, Slot) ->
    Flags = case S of true -> 1; false -> 0 end,
    <<Server:32/little, ?MSG_AER_REPLY:8, (Slot(Peer)):8, Flags:8, 0:8, T:64/little,
      NI:64/little, LI:64/little, (term_or_undef(LT)):64/little, 0:64, 0:64, 0:64>>;
encode_msg(Server, #request_vote_rpc{term = T, candidate_id = C, last_log_index = LLI,
                                     last_log_term = LLT}, Slot) ->
    <<Server:32/little, ?MSG_REQUEST_VOTE:8, (Slot(C)):8, 0:8, 0:8, T:64/little, LLI:64/little,
      LLT:64/little, 0:64, 0:64, 0:64, 0:64>>;
encode_msg(Server, {ra_log_event, {written, T, Seq}}, _Slot) ->
    %% the written event carries a ra_seq:state() -- a list of indexes and ranges, newest first
    %% (src/ra_log_wal.erl:807, src/ra_log.erl:74,1641; ra_seq.erl:8-12) -- e.g. [{From,To}], [Idx],
    %% {written,0,[0]} or, after ra_log:write_sparse/3, something like [14, {2,9}].  One range, or two
    %% (RGB_MF_SEQ2 = 8: the lower one rides in the run0_term/run1_term fields), fit the record.  A longer
    %% sequence (ABI v8, RGB_MF_SEQX = 32) keeps its two highest ranges in the record and names the others in
    %% the batch's range list: {seqx, Record, LowerRanges} -- the record's `c` (first list entry) is filled in
    %% by encode_msgs/2, which knows where the batch's list stands.  No written event falls back any more.
    case seq_ranges(Seq) of
        [{From, To}] ->
            <<Server:32/little, ?MSG_WRITTEN:8, ?NONE:8, 0:8, 0:8, T:64/little, From:64/little,
              To:64/little, 0:64, 0:64, 0:64, 0:64>>;
        [{From2, To2}, {From, To}] ->
            <<Server:32/little, ?MSG_WRITTEN:8, ?NONE:8, 8:8, 0:8, T:64/little, From:64/little,
              To:64/little, 0:64, 0:64, From2:64/little, To2:64/little>>;
        Ranges ->
            {Lower, [{From2, To2}, {From, To}]} = lists:split(length(Ranges) - 2, Ranges),
            {seqx,
             fun(C) ->
                     <<Server:32/little, ?MSG_WRITTEN:8, ?NONE:8, (8 bor 32):8, 0:8, T:64/little, From:64/little,
                       To:64/little, C:64/little, (length(Lower)):32/little, 0:32, From2:64/little, To2:64/little>>
             end,
             << <<F:64/little, L:64/little>> || {F, L} <- Lower >>}
    end;
encode_msg(Server, {Peer, #request_vote_result{term = T, vote_granted = G}}, Slot) ->
    Flags = case G of true -> 1; false -> 0 end,
    <<Server:32/little, ?MSG_VOTE_RESULT:8, (Slot(Peer)):8, Flags:8, 0:8, T:64/little, 0:(6 * 64)>>;
encode_msg(Server, #pre_vote_rpc{version = V, machine_version = MV, term = T, token = Tok, candidate_id = C,
                                 last_log_index = LLI, last_log_term = LLT}, Slot) ->
    %% the token is a reference in the reference; the caller maps it to a 64-bit integer (erlang:phash2 of the
    %% ref is NOT unique enough: keep a per-server counter and a map Ref -> integer beside the gen_statem)
    <<Server:32/little, ?MSG_PRE_VOTE_RPC:8, (Slot(C)):8, 0:8, V:8, T:64/little, LLI:64/little,
      LLT:64/little, Tok:64/little, MV:32/little, 0:32, 0:64, 0:64>>;
encode_msg(Server, {Peer, #pre_vote_result{term = T, token = Tok, vote_granted = G}}, Slot) ->
    Flags = case G of true -> 1; false -> 0 end,
    <<Server:32/little, ?MSG_PRE_VOTE_RESULT:8, (Slot(Peer)):8, Flags:8, 0:8, T:64/little, 0:64, 0:64,
      Tok:64/little, 0:64, 0:64, 0:64>>;
encode_msg(Server, {election_timeout, Tok}, _Slot) ->
    %% election_timeout in follower / pre_vote / candidate; Tok = the integer standing for make_ref() of
    %% call_for_election(pre_vote, ..) (src/ra_server.erl:2900-2924)
    <<Server:32/little, ?MSG_ELECTION_TIMEOUT:8, ?NONE:8, 0:8, 0:8, 0:64, 0:64, 0:64, Tok:64/little,
      0:64, 0:64, 0:64>>;
encode_msg(Server, {commands, NEntries, Force}, _Slot) ->
    %% {command, _} / {commands, _} on the leader: only the COUNT crosses (payloads go to ra_log:append on the
    %% host, src/ra_server.erl:653-738); Force = true for the noop of a new term (RGB_MF_FORCE = 2)
    Flags = case Force of true -> 2; false -> 0 end,
    <<Server:32/little, ?MSG_APPEND:8, ?NONE:8, Flags:8, 0:8, 0:64, 0:64, 0:64, 0:64,
      NEntries:32/little, 0:32, 0:64, 0:64>>;
encode_msg(Server, await_condition_timeout, _Slot) ->
    <<Server:32/little, ?MSG_AWAIT_TIMEOUT:8, ?NONE:8, 0:8, 0:8, 0:(7 * 64)>>;
encode_msg(Server, {ra_log_event, {snapshot_written, {Idx, T}, _, snapshot, _, _}}, _Slot) ->
    <<Server:32/little, ?MSG_SNAPSHOT_WRITTEN:8, ?NONE:8, 0:8, 0:8, 0:64, Idx:64/little,
      T:64/little, 0:64, 0:64, 0:64, 0:64>>;
encode_msg(Server, #heartbeat_rpc{term = T, leader_id = L, query_index = QI}, Slot) ->
    <<Server:32/little, ?MSG_HEARTBEAT_RPC:8, (Slot(L)):8, 0:8, 0:8, T:64/little, QI:64/little,
      0:(5 * 64)>>;
encode_msg(Server, {Peer, #heartbeat_reply{term = T, query_index = QI}}, Slot) ->
    <<Server:32/little, ?MSG_HEARTBEAT_REPLY:8, (Slot(Peer)):8, 0:8, 0:8, T:64/little,
      QI:64/little, 0:(5 * 64)>>;
encode_msg(Server, {consistent_query, _From, _Fun}, _Slot) ->
    %% only while cluster_change_permitted; the QueryRef is queued by the caller under the
    %% query index the decision returns (reply_last_term)
    <<Server:32/little, ?MSG_CONSISTENT_QUERY:8, ?NONE:8, 0:8, 0:8, 0:(7 * 64)>>;
encode_msg(Server, {transfer_leadership, Target}, Slot) ->
    %% the leader_call of ra:transfer_leadership/2 (src/ra.erl:1156-1173); Slot(Target) = 255 for a server id that is
    %% not a key of the cluster map (the device answers unknown_member)
    <<Server:32/little, ?MSG_TRANSFER_LEADERSHIP:8, (Slot(Target)):8, 0:8, 0:8, 0:(7 * 64)>>;
encode_msg(Server, pipeline_rpcs, _Slot) ->
    <<Server:32/little, ?MSG_PIPELINE_RPCS:8, ?NONE:8, 0:8, 0:8, 0:(7 * 64)>>;
encode_msg(Server, tick_timeout, _Slot) ->
    %% leader(_, tick_timeout, _) -> make_rpcs/1 (src/ra_server_proc.erl:613-616): RGB_MF_TICK = 4
    <<Server:32/little, ?MSG_PIPELINE_RPCS:8, ?NONE:8, 4:8, 0:8, 0:(7 * 64)>>.

entry_runs(_PI, []) -> {0, 0, 0, 0, 0};
entry_runs(PI, [{I0, T0, _} | _] = Es) ->
    {Run0, Rest} = lists:splitwith(fun({_, T, _}) -> T =:= T0 end, Es),
    T1 = case Rest of [] -> 0; [{_, T, _} | _] -> T end,
    true = lists:all(fun({_, T, _}) -> T =:= T1 end, Rest), %% else: fall back to ra_server
    {length(Es), length(Run0), T0, T1, I0 - (PI + 1)}.

%% a ra_seq as ascending, merged {Lo, Hi} ranges
seq_ranges(Seq) ->
    lists:reverse(ra_seq:fold(fun (I, [{Lo, Hi} | R]) when I =:= Hi + 1 -> [{Lo, I} | R];
                                  (I, Acc) -> [{I, I} | Acc]
                              end, [], Seq)).

term_or_undef(undefined) -> ?UNDEF;
term_or_undef(T) -> T.

decode_decision(<<Server:32/little, Role:8, ReplyTo:8, NRpcs:8, Kind:8, Flags:32/little,
                  Inv:16/little, HbTo:8, Cancel:8, RT:64/little, RNI:64/little, RLI:64/little, RLT:64/little,
                  CI:64/little, LA:64/little>>) ->
    #{server => Server, role => role(Role), reply_to => ReplyTo, n_rpcs => NRpcs, kind => Kind,
      flags => Flags, invariant => Inv, heartbeat_to => HbTo, cancel_backoff => Cancel, reply_term => RT, reply_next_index => RNI,
      reply_last_index => RLI, reply_last_term => RLT, commit_index => CI, last_applied => LA}.

role(0) -> follower; role(1) -> candidate; role(2) -> leader; role(3) -> pre_vote;
role(4) -> await_condition.

%% Reconstitute the effects() list ra_server_proc:handle_effects/4 expects from a decision
%% (reference src/ra_server.erl:178-206 for the vocabulary).  Id = this server's id,
%% Member = fun(Slot) -> ra_server_id(); Member(first_peer) = the first key of the cluster map without Id
%% (only asked for with F_TRANSFER_LEADERSHIP); Member(call) = the call message the decision answers (only asked for
%% with F_CALL_REPLY and ?CALL_UNSUPPORTED).
decision_to_effects(Id, Member, #{flags := F} = D) when F band ?F_INVARIANT =/= 0 ->
    %% the reference would have exited: do exactly that (reason by code, see the header)
    exit({ra_gpu_batch_invariant, Id, maps:get(invariant, D), Member});
decision_to_effects(_Id, Member, #{flags := F, reply_next_index := Code, reply_to := To})
  when F band ?F_CALL_REPLY =/= 0 ->
    %% handle_leader({transfer_leadership, Target}, _) src/ra_server.erl:996-1035, in the reference's order; the
    %% other roles' catch-all clause (:1186-1188, 1276-1278, 1655-1657).  The twin of ra_amd/effects.py call_reply/2
    case Code of
        ?CALL_OK -> [{reply, ok}, {send_msg, Member(To), election_timeout, cast}];
        ?CALL_ALREADY_LEADER -> [{reply, already_leader}];
        ?CALL_UNKNOWN_MEMBER -> [{reply, {error, unknown_member}}];
        ?CALL_NON_VOTER -> [{reply, {error, non_voter}}];
        ?CALL_NOT_UP_TO_DATE -> [{reply, {error, not_up_to_date}}];
        ?CALL_UNSUPPORTED -> [{reply, {error, {unsupported_call, Member(call)}}}]
    end;
decision_to_effects(Id, Member, #{flags := F, reply_to := To} = D) ->
    Reply =
        if F band ?F_REPLY =:= 0 -> [];
           F band ?F_REPLY_VOTE =/= 0 ->
               [{reply, #request_vote_result{term = maps:get(reply_term, D),
                                             vote_granted = F band ?F_REPLY_SUCCESS =/= 0}}];
           F band ?F_REPLY_HEARTBEAT =/= 0 ->
               [{cast, Member(To),
                 {Id, #heartbeat_reply{term = maps:get(reply_term, D),
                                       query_index = maps:get(reply_next_index, D)}}}];
           F band ?F_REPLY_PRE_VOTE =/= 0 ->
               [{reply, {pre_vote_result, maps:get(reply_term, D), maps:get(reply_next_index, D),
                         F band ?F_REPLY_SUCCESS =/= 0}}];
           true ->
               [{cast, Member(To),
                 {Id, #append_entries_reply{term = maps:get(reply_term, D),
                                            success = F band ?F_REPLY_SUCCESS =/= 0,
                                            next_index = maps:get(reply_next_index, D),
                                            last_index = maps:get(reply_last_index, D),
                                            last_term = maps:get(reply_last_term, D)}}}]
        end,
    Heartbeats =
        [{send_rpc, Member(Slot),
          #heartbeat_rpc{term = maps:get(reply_term, D), leader_id = Id,
                         query_index = maps:get(reply_last_term, D)}}
         || F band ?F_SEND_HEARTBEATS =/= 0, Slot <- lists:seq(0, 7),
            maps:get(heartbeat_to, D) band (1 bsl Slot) =/= 0],
    %% F_QUERY_QUORUM: release queued queries with index =< reply_next_index (the caller owns
    %% queries_waiting_heartbeats); F_QUERY_APPLY: no peers, apply now; F_RESEND_PENDING:
    %% ra_log:resend_pending/2 on the host log
    Cancels =
        [{cancel_snapshot_retry_timer, Member(Slot)}
         || F band ?F_CANCEL_SNAPSHOT_RETRY =/= 0, Slot <- lists:seq(0, 7),
            maps:get(cancel_backoff, D) band (1 bsl Slot) =/= 0],
    Cancels ++ Reply ++ Heartbeats
    ++ [{record_leader_msg, Member(To)} || F band ?F_LEADER_MSG =/= 0]
    ++ [{next_event, info, pipeline_rpcs} || F band ?F_PIPELINE =/= 0]
    ++ [{aux, eval} || F band ?F_AUX_EVAL =/= 0]
    %% the leader's wal_down condition timed out with the WAL still down (ra_server.erl:660-668): Member(first_peer)
    %% must resolve to hd(maps:to_list(maps:remove(Id, Cluster))) -- the caller's Member fun knows the cluster map
    ++ [{next_event, cast, {transfer_leadership, Member(first_peer)}} || F band ?F_TRANSFER_LEADERSHIP =/= 0].
