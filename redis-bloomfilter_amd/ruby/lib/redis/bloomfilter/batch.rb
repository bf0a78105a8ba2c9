# frozen_string_literal: true

# Batched delegators for Redis::Bloomfilter (lib/redis/bloomfilter.rb:61-73
# gains two siblings).  Drivers with a batch path (hip) get one call per batch;
# the ruby and lua drivers keep working through the per-key loop.
class Redis
  class Bloomfilter
    def insert_many(keys, expire = nil)
      expire ||= @options[:default_expire]
      return @driver.insert_many(keys, expire) if @driver.respond_to?(:insert_many)

      keys.each { |k| @driver.insert(k, expire) }
      nil
    end

    def include_many?(keys)
      return @driver.include_many?(keys) if @driver.respond_to?(:include_many?)

      keys.map { |k| @driver.include?(k) }
    end

    # Statistics and merging (the hip drivers: BITCOUNT / BITOP OR on the device string).
    # A driver without them raises NotImplementedError naming itself.
    def count_bits
      stats_driver(:count_bits).count_bits
    end

    def fill_ratio
      stats_driver(:fill_ratio).fill_ratio
    end

    def estimated_size
      stats_driver(:estimated_size).estimated_size
    end

    def merge(other, expire = nil)
      expire ||= @options[:default_expire]
      stats_driver(:merge).merge(other.driver, expire)
    end

    def union_size(other)
      stats_driver(:union_size).union_size(other.driver)
    end

    def intersection_size(other)
      stats_driver(:intersection_size).intersection_size(other.driver)
    end

    private

    def stats_driver(name)
      return @driver if @driver.respond_to?(name)

      raise NotImplementedError, "driver '#{@options[:driver]}' has no #{name}"
    end
  end
end
